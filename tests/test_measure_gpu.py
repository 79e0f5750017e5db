"""k_measure_maxrgb (extension: the histogram of max(R, G, B) of rendered frames, include/mpcvr.h) on the GPU: both instantiations word for
word against the numpy model (tests/measure_model.py) over the shapes where a four-column lane can go wrong, exact large counts, what is
written around the histogram, the refusals, mpcvr_measure_backbuffer, an HDR10 frame end to end and mpcvr_process_batch_yuv_stats.
The host functions: tests/test_measure.py (CPU)."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import encode_model as EM
from tests import measure_model as MM
from tests.golden.cases import HDR10, M709, MPEG2, TV, case_frame, ext
from tests.test_batch_yuv_gpu import new_planes, noise_frames
from tests.test_encode_gpu import NV12, P010, description
from tests.test_parity_gpu import make_vp

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = MM.BGRA8, MM.RGB10A2
BINS = MM.BINS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def band_rows():
    text = open(os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_measure.h")).read()
    return int(re.search(r"constexpr\s+int\s+kMeasureBandRows\s*=\s*(\d+)\s*;", text).group(1))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def counts(t):
    """a device tensor of int32 words holding uint32 counts -> int64 numpy"""
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def device_words(ptr, n):
    out = np.empty(n, dtype=np.uint32)
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0      # hipMemcpyDeviceToHost
    return out


def texels(rng, shape, src_fmt, top):
    """uint32 texels with each code field drawn from [0, top] and random A / X bits"""
    bits = 10 if src_fmt == RGB10A2 else 8
    f = [rng.integers(0, top + 1, size=shape, dtype=np.uint64) for _ in range(3)]
    a = rng.integers(0, 1 << (32 - 3 * bits), size=shape, dtype=np.uint64)
    return (f[0] | f[1] << bits | f[2] << (2 * bits) | a << (3 * bits)).astype(np.uint32)


# ---- 1. both instantiations equal the model over a thinned sweep ------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 259)
LEFTS = (0, 1, 2, 3, 5)
PITCH_PADS = (0, 4, 16, 20)
BASES = (0, 4, 8)


def sweep_configs():
    """(rect width, left, height, pitch pad, base, top, right margin): every (width, left) pair once, with heights, pitches and bases taking
    turns; then every (height, pitch pad, base) triple once, with the (width, left) pairs taking turns.  Even configurations get a surface
    whose width is a multiple of 4 (a tight pitch on 16 bytes: the 16-byte loads), odd ones end the surface at the rectangle's right edge
    (the lane that holds the last columns of a width that is no multiple of 4)."""
    B = band_rows()
    heights = (1, 2, 3, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1)
    pairs = [(w, l) for w in WIDTHS for l in LEFTS]
    triples = [(h, p, b) for h in heights for p in PITCH_PADS for b in BASES]
    out = []
    for k, (w, l) in enumerate(pairs):
        h, p, b = triples[(k * 7) % len(triples)]
        out.append((w, l, h, p, b))
    for k, (h, p, b) in enumerate(triples):
        w, l = pairs[(k * 11 + 3) % len(pairs)]
        out.append((w, l, h, p, b))
    full = []
    for k, (w, l, h, p, b) in enumerate(out):
        top = k % 3
        margin = (-(l + w)) % 4 if k % 2 == 0 else 0
        full.append((w, l, h, p, b, top, margin))
    # ... and every (width, left) pair once more on the 16-byte loads: the surface ends at the rectangle's right edge, the pitch is padded
    # to a multiple of 16 (so a width that is no multiple of 4 leaves its last columns to a lane that must fall back to dword loads)
    for k, (w, l) in enumerate(pairs):
        full.append((w, l, heights[k % len(heights)], (-4 * (l + w)) % 16 + 16 * (k & 1), 0, k % 2, 0))
    return full


@pytest.mark.parametrize("src_fmt", [BGRA8, RGB10A2], ids=["bgra8", "rgb10a2"])
def test_both_instantiations_equal_the_model_word_for_word(mpcvr, torch_cuda, src_fmt):
    """Inside the rectangle: codes from [0, maxin - 1] with random A / X bits (first draw), full-range noise (second draw).  Every texel
    outside the rectangle and all pitch padding is 0xFFFFFFFF: a read outside the rectangle lands in bin maxin, which the first draw keeps 0."""
    from videorenderer_amd import api
    torch = torch_cuda
    top_code = MM.maxin(src_fmt)
    hist = torch.empty(BINS, dtype=torch.int32, device="cuda")
    vec = dword = 0
    for k, (w, l, h, pad, base, top, margin) in enumerate(sweep_configs()):
        sw, sh = l + w + margin, top + h + (k % 2)
        pitch = sw * 4 + pad
        rect = (l, top, l + w, top + h)
        for draw in (0, 1):
            rng = np.random.default_rng(10000 * draw + 10 * k + src_fmt)
            surface = np.full((sh, sw), 0xffffffff, dtype=np.uint32)
            surface[top:top + h, l:l + w] = texels(rng, (h, w), src_fmt, top_code - 1 if draw == 0 else top_code)
            host = np.full(base + sh * pitch + 64, 0xff, dtype=np.uint8)
            rows = host[base:base + sh * pitch].reshape(sh, pitch)
            rows[:, :sw * 4] = surface.view(np.uint8).reshape(sh, sw * 4)
            dev = torch.from_numpy(host).cuda()
            assert dev.data_ptr() % 16 == 0
            hist.fill_(0x5a5a5a5a)
            api.measure_pass(dev.data_ptr() + base, pitch, src_fmt, sw, sh, hist, rect)
            torch.cuda.synchronize()
            got, want = counts(hist), MM.hist(surface, src_fmt, rect)
            what = "rect %s of %dx%d, pitch %d, base +%d, draw %d" % (rect, sw, sh, pitch, base, draw)
            assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].ravel(), got[got != want][:6], want[got != want][:6])
            if draw == 0:
                assert got[top_code] == 0 and got.sum() == w * h, what
        if base % 16 == 0 and pitch % 16 == 0:
            vec += 1
        else:
            dword += 1
    assert vec >= 20 and dword >= 20, (vec, dword)          # both load paths ran


# ---- 2. exact large counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_fmt", [BGRA8, RGB10A2], ids=["bgra8", "rgb10a2"])
def test_counts_above_2_24_are_exact(mpcvr, torch_cuda, src_fmt):
    """4096 x 4100 texels of one code: that bin is w * h = 16 793 600 exactly (a float accumulator, a 16-bit packed counter or a lost
    same-address add would miss it), every other bin 0; then the frame split between two codes down a column that is no multiple of 4."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h = 4096, 4100
    top = MM.maxin(src_fmt)
    bits = 10 if src_fmt == RGB10A2 else 8
    alpha = (0xffffffff << (3 * bits)) & 0xffffffff
    zero, full = alpha, (top << bits)                     # code 0 with every A / X bit set; maxin in G alone
    as_i32 = lambda v: int(np.array(v, dtype=np.uint32).view(np.int32))
    surface = torch.empty((h, w), dtype=torch.int32, device="cuda")
    hist = torch.empty(BINS, dtype=torch.int32, device="cuda")
    for code, word in ((0, zero), (top, full)):
        surface.fill_(as_i32(word))
        hist.fill_(-1)
        api.measure_pass(surface, w * 4, src_fmt, w, h, hist)
        torch.cuda.synchronize()
        got = counts(hist)
        assert got[code] == w * h == 16793600, (code, got[code])
        assert got.sum() == w * h, (code, np.nonzero(got)[0][:8])
    split = 1001
    low = 37 << (2 * bits) | 5                            # max(R, G, B) == 37
    surface[:, :split] = as_i32(low | alpha)
    api.measure_pass(surface, w * 4, src_fmt, w, h, hist)
    torch.cuda.synchronize()
    got = counts(hist)
    assert got[37] == split * h and got[top] == (w - split) * h and got.sum() == w * h, (got[37], got[top], got.sum())


# ---- 3. the histogram is overwritten and nothing else is touched -------------------------------------------------------------------------
def test_the_histogram_is_overwritten_and_nothing_else_is_written(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    w, h = 259, 70
    rng = np.random.default_rng(5)
    surface = texels(rng, (h, w), RGB10A2, 1023)
    dev = torch.from_numpy(surface.view(np.int32)).cuda()
    before = dev.clone()
    guard = 256
    i = torch.arange(guard + BINS + guard, dtype=torch.int32, device="cuda")
    pattern = i * 40503 + 977
    buf = pattern.clone()
    hist = buf[guard:guard + BINS]
    results = []
    for garbage in (0x7fffffff, -3):
        hist.fill_(garbage)
        api.measure_pass(dev, w * 4, RGB10A2, w, h, hist, (1, 2, 258, 69))
        torch.cuda.synchronize()
        results.append(counts(hist))
        assert torch.equal(buf[:guard], pattern[:guard]) and torch.equal(buf[guard + BINS:], pattern[guard + BINS:]), "a word beside the histogram was written"
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], MM.hist(surface, RGB10A2, (1, 2, 258, 69)))
    assert torch.equal(dev, before), "the surface was written"


# ---- 4. refusals write nothing ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h = 16, 8
    pitch = w * 4 + 16
    buf = torch.full((h * pitch + BINS * 4 + 64,), 0x5a, dtype=torch.uint8, device="cuda")
    s0 = buf.data_ptr()
    h0 = s0 + h * pitch + 32                               # behind the surface

    def call(s=s0, sp=pitch, fmt=BGRA8, w=w, h=h, rect="whole", hist=h0):
        r = None if rect == "whole" else C.byref(api.Rect(*rect))
        return L.mpcvr_measure_pass(C.c_void_p(s), sp, fmt, w, h, r, C.c_void_p(hist), None)

    E, Pn = api.E_INVALIDARG, api.E_POINTER
    last = s0 + (h - 1) * pitch + w * 4                    # one past the last pixel of the last row
    for kw, hr in ((dict(s=None), Pn), (dict(hist=None), Pn),
                   (dict(fmt=2), E), (dict(fmt=-1), E),
                   (dict(w=0), E), (dict(h=0), E), (dict(w=32769, sp=4 * 32769 + 3), E), (dict(h=32769), E),
                   (dict(s=s0 + 2), E), (dict(sp=pitch + 2), E), (dict(sp=w * 4 - 4), E), (dict(hist=h0 + 2), E),
                   (dict(rect=(4, 2, 4, 6)), E), (dict(rect=(4, 6, 8, 6)), E), (dict(rect=(8, 2, 4, 6)), E),        # empty
                   (dict(rect=(-1, 0, 4, 4)), E), (dict(rect=(0, -1, 4, 4)), E), (dict(rect=(0, 0, w + 1, 4)), E), (dict(rect=(0, 0, 4, h + 1)), E),
                   (dict(hist=last - 4), E),                # the histogram starts on the last pixel
                   (dict(hist=s0), E),
                   (dict(s=s0 + BINS * 4 - 4, hist=s0), E)):          # the surface starts on the histogram's last word
        assert call(**kw) == hr, kw
    torch.cuda.synchronize()
    assert bool((buf == 0x5a).all()), "a refused call wrote"
    # ... and the arguments they were derived from are accepted; a histogram that merely touches the surface's last pixel, too
    assert call(hist=last, rect=(1, 1, w, h)) == 0 and call() == 0
    torch.cuda.synchronize()
    got = counts(buf[h * pitch + 32:h * pitch + 32 + BINS * 4].view(torch.int32))
    assert got[0x5a] == w * h and got.sum() == w * h


# ---- 5. mpcvr_measure_backbuffer ------------------------------------------------------------------------------------------------------------
LETTERBOX = dict(cformat=1, w=96, h=64, kind="structure", seed=91, exfmt=ext(matrix=M709), iUpscaling=2, dst=(77, 57), window=(96, 64), offset=(9, 3))
ACTIVE = (9, 3, 86, 60)


def backbuffer_words(vp):
    ptr, pitch, w, h = vp.GetBackBuffer()
    assert pitch == w * 4
    return device_words(ptr, w * h).reshape(h, w)


@pytest.mark.parametrize("out_fmt", [BGRA8, RGB10A2], ids=["bgra8", "rgb10a2"])
def test_measure_backbuffer_counts_the_active_picture(mpcvr, torch_cuda, out_fmt):
    from videorenderer_amd import api
    torch = torch_cuda
    c = dict(LETTERBOX, output_format=out_fmt)
    vp, (ww, wh) = make_vp(mpcvr, c)
    hist = torch.full((BINS,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    assert vp._L.mpcvr_measure_backbuffer(vp._ctx, C.c_void_p(hist.data_ptr())) == api.S_FALSE          # nothing rendered yet
    vp.Synchronize()
    assert bool((hist == 0x5a5a5a5a).all())
    frame, pitch = case_frame(c)
    dev = torch.from_numpy(frame).cuda()
    vp.CopySample(dev, pitch)
    area = (ACTIVE[2] - ACTIVE[0]) * (ACTIVE[3] - ACTIVE[1])
    for how in ("render", "render_yuv"):
        if how == "render":
            assert vp.Render(1) == 0
        else:
            vp.RenderYuv(NV12, ext(MPEG2, TV, M709))
        hist.fill_(-1)
        torch.cuda.synchronize()
        assert vp.MeasureBackBuffer(hist) is hist
        vp.Synchronize()
        got = counts(hist)
        back = backbuffer_words(vp)
        ll = api.light_level_from_histogram(got, out_fmt)
        assert ll["pixels"] == area, (how, ll, "the window holds %d texels" % (ww * wh))
        assert np.array_equal(got, MM.hist(back, out_fmt, ACTIVE)), how
        assert not MM.max_rgb(back[:3], out_fmt).any() and not MM.max_rgb(back[:, :9], out_fmt).any()          # the letterbox is black
        assert ll["max_code"] > ll["min_code"]
    # an empty active area (the video rect moved off the window behind the render): zeros, S_OK
    vp.SetVideoRect((200, 200, 260, 240))
    hist.fill_(-1)
    torch.cuda.synchronize()
    assert vp._L.mpcvr_measure_backbuffer(vp._ctx, C.c_void_p(hist.data_ptr())) == 0
    vp.Synchronize()
    assert not bool(hist.any())
    # refusals
    assert vp._L.mpcvr_measure_backbuffer(vp._ctx, None) == api.E_POINTER
    assert vp._L.mpcvr_measure_backbuffer(vp._ctx, C.c_void_p(hist.data_ptr() + 2)) == api.E_INVALIDARG
    assert vp._L.mpcvr_measure_backbuffer(vp._ctx, C.c_void_p(vp.GetBackBuffer()[0])) == api.E_INVALIDARG
    vp.close()


def test_measure_backbuffer_is_ordered_between_two_renders_on_the_lanes(mpcvr, torch_cuda):
    """A context that owns its stream renders on its frame lanes: render A, measure, render B (another sample, into the same back buffer),
    then synchronise — the histogram belongs to A.  Several rounds, so that both lanes take both roles."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = LETTERBOX
    kw = {k: c[k] for k in ("iUpscaling",)}
    vp = api.VideoProcessor(api.default_settings(**kw), use_torch_stream=False)
    vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c["exfmt"])
    vp.SetWindowRect((0, 0) + c["window"])
    vp.SetVideoRect(ACTIVE)
    samples = []
    for seed, kind in ((92, "structure"), (93, "noise")):
        frame, pitch = case_frame(dict(c, seed=seed, kind=kind))
        samples.append(torch.from_numpy(frame).cuda())
    torch.cuda.synchronize()
    want = []
    for s in samples:                                       # each sample's histogram on its own, everything synchronised
        vp.CopySample(s, pitch)
        assert vp.Render(1) == 0
        vp.Synchronize()
        want.append(MM.hist(backbuffer_words(vp), BGRA8, ACTIVE))
    assert not np.array_equal(want[0], want[1])
    hists = torch.zeros((8, BINS), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for r in range(8):
        vp.CopySample(samples[r & 1], pitch)
        assert vp.Render(1) == 0
        assert vp.MeasureBackBuffer(hists[r]) is not None
        vp.CopySample(samples[1 - (r & 1)], pitch)
        assert vp.Render(1) == 0
    vp.Synchronize()
    for r in range(8):
        assert np.array_equal(counts(hists[r]), want[r & 1]), "round %d: the histogram is not the frame's that was rendered in front of it" % r
    vp.close()


# ---- 6. HDR10 end to end -------------------------------------------------------------------------------------------------------------------
def test_hdr10_passthrough_light_levels(mpcvr, torch_cuda):
    """A P010 PQ sample of four flat patches, passed through (mpcvr_set_hdr_output(1, 0, ...)) into RGB10A2: the codes and nits from the
    histogram equal the model on the frame read back, and max_nits is L of the brightest patch's code in that frame."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h = 64, 32
    luma = (80, 300, 520, 769)                              # 10-bit codes, limited range
    y = np.repeat(np.array(luma, dtype=np.uint16) << 6, w // 4)[None, :].repeat(h, 0)
    uv = np.full((h // 2, w), 512 << 6, dtype=np.uint16)
    sample = torch.from_numpy(np.concatenate([y.reshape(-1), uv.reshape(-1)]).view(np.uint8).copy()).cuda()
    vp = api.VideoProcessor(api.default_settings(output_format=RGB10A2, bUseDither=0))
    vp.InitMediaType(P010, w, h, pitch=w * 2, extfmt=HDR10)
    vp.SetWindowRect((0, 0, w, h))
    vp.SetVideoRect((0, 0, w, h))
    vp.SetHdrOutput(True, 0, 1000.0)
    vp.CopySample(sample, w * 2)
    assert vp.Render(1) == 0
    hist = vp.MeasureBackBuffer()
    vp.Synchronize()
    got = api.light_level_from_histogram(counts(hist), RGB10A2)
    back = backbuffer_words(vp)
    codes = MM.max_rgb(back, RGB10A2)
    want = MM.light_level(MM.hist(back, RGB10A2), RGB10A2)
    rtol = 1e-11                                            # tests/test_measure.py: NITS_RTOL, with its derivation
    assert (got["pixels"], got["min_code"], got["max_code"]) == (w * h, want["min_code"], want["max_code"])
    assert abs(got["avg_nits"] - float(want["avg_nits"])) <= rtol * float(want["avg_nits"])
    brightest = int(codes[:, 3 * w // 4:].max())
    assert brightest == int(codes.max()) == got["max_code"] and int(codes[:, :w // 4].max()) < brightest
    assert abs(got["max_nits"] - float(MM.pq_nits(brightest, RGB10A2))) <= rtol * got["max_nits"]
    print("HDR10 passthrough: patches", luma, "-> codes", sorted(set(codes.reshape(-1).tolist())), "MaxCLL %.3f nits, FALL %.3f nits" % (got["max_nits"], got["avg_nits"]))
    assert 0.0 < got["avg_nits"] < got["max_nits"] <= 10000.0
    vp.close()


# ---- 7. mpcvr_process_batch_yuv_stats -----------------------------------------------------------------------------------------------------
# exact 2x, 128 x 18 -> 256 x 36 at (1, 1) of a 258 x 38 window (the case of tests/test_batch_yuv_gpu.py: a lane route, with a letterbox)
BATCH_CASE = dict(cformat=2, w=128, h=18, kind="noise", seed=811, dst=(256, 36), window=(258, 38), offset=(1, 1), exfmt=HDR10, iUpscaling=4)
BATCH_ACTIVE = (1, 1, 257, 37)


def stats_context(mpcvr, torch, own):
    from videorenderer_amd import api
    c = BATCH_CASE
    if not own:
        return make_vp(mpcvr, c)[0]
    vp = api.VideoProcessor(api.default_settings(iUpscaling=c["iUpscaling"]), use_torch_stream=False)
    vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c["exfmt"])
    vp.SetWindowRect((0, 0) + c["window"])
    vp.SetVideoRect(BATCH_ACTIVE)
    return vp


def test_batch_yuv_stats(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    c = BATCH_CASE
    ww, wh = c["window"]
    n = 5
    desc = description(NV12, EM.LEFT)
    frames = noise_frames(torch, c, n)
    others = noise_frames(torch, c, n, seed0=50)
    budget = 2 * api.plan_batch_yuv(ww, wh, n, 0)["frame_stride"]
    assert api.plan_batch_yuv(ww, wh, n, budget)["chunks"] == 3

    # the reference: the plain call's planes and launch count; mpcvr_measure_pass over the active rect of mpcvr_process_batch's targets
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                              # (torch's default stream is NULL = "the context's own stream")
    with torch.cuda.stream(side):
        ref = stats_context(mpcvr, torch, False)
    ref.SetBatchYuvBudget(budget)
    want_y, want_uv, pitch = new_planes(torch, n, ww, wh, False)
    torch.cuda.synchronize()
    ref.ProcessBatchYuv(frames, NV12, desc, want_y, pitch, want_uv, pitch)
    ref.Synchronize()
    plain = ref.GetLastBatchInfo()
    assert plain["yuv_chunks"] == 3
    want_rows = []
    for fs in (frames, others):
        rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in fs]
        torch.cuda.synchronize()
        ref.ProcessBatch(fs, rgb, ww * 4)
        ref.Synchronize()
        rows = torch.zeros((n, BINS), dtype=torch.int32, device="cuda")
        for i, t in enumerate(rgb):
            api.measure_pass(t, ww * 4, BGRA8, ww, wh, rows[i], BATCH_ACTIVE)
        torch.cuda.synchronize()
        want_rows.append(counts(rows))
        for i, t in enumerate(rgb):                       # ... which is the model's (the test does not rest on the library alone)
            assert np.array_equal(want_rows[-1][i], MM.hist(t.cpu().numpy().view(np.uint32).reshape(wh, ww), BGRA8, BATCH_ACTIVE)), i
    area = (BATCH_ACTIVE[2] - BATCH_ACTIVE[0]) * (BATCH_ACTIVE[3] - BATCH_ACTIVE[1])
    assert (want_rows[0].sum(1) == area).all() and not np.array_equal(want_rows[0][0], want_rows[0][1])

    results = {}
    for own in (False, True):
        with (contextlib.nullcontext() if own else torch.cuda.stream(side)):
            vp = stats_context(mpcvr, torch, own)
        vp.SetBatchYuvBudget(budget)
        ys, uvs, _ = new_planes(torch, n, ww, wh, False)
        rows = torch.full((n, BINS), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        vp.ProcessBatchYuvStats(frames, NV12, desc, ys, pitch, uvs, pitch, rows)
        vp.Synchronize()
        info = vp.GetLastBatchInfo()
        assert info["yuv_chunks"] == 3 and info["launches"] == plain["launches"] + 3, (own, info, plain)
        if own and os.environ.get("MPCVR_NO_BATCH_LANES") != "1":
            assert {0, 1} <= set(info["yuv_lanes"]), info          # (chunks of 2, 2 and 1: the chunks of two take turns on the lanes)
        for i in range(n):
            assert torch.equal(ys[i], want_y[i]) and torch.equal(uvs[i], want_uv[i]), (own, "planes of frame %d differ from mpcvr_process_batch_yuv" % i)
        got = counts(rows)
        assert np.array_equal(got, want_rows[0]), (own, np.argwhere(got != want_rows[0])[:6])
        results[own] = got
        # two consecutive calls with different samples into the SAME rows and planes: the second call's are left
        vp.ProcessBatchYuvStats(frames, NV12, desc, ys, pitch, uvs, pitch, rows)
        vp.ProcessBatchYuvStats(others, NV12, desc, ys, pitch, uvs, pitch, rows)
        vp.Synchronize()
        assert np.array_equal(counts(rows), want_rows[1]), (own, "rows of the first of two calls survived")
        # refusals: planes and rows untouched
        L = vp._L
        arr = C.c_void_p * n
        sa, ya, ua = arr(*[f.data_ptr() for f in frames]), arr(*[t.data_ptr() for t in ys]), arr(*[t.data_ptr() for t in uvs])
        keep_rows, keep_y, keep_uv = rows.clone(), [t.clone() for t in ys], [t.clone() for t in uvs]
        torch.cuda.synchronize()

        def call(hist):
            return L.mpcvr_process_batch_yuv_stats(vp._ctx, n, sa, NV12, desc, ya, pitch, ua, pitch, C.c_void_p(hist) if hist is not None else None)

        assert call(None) == api.E_POINTER
        assert call(rows.data_ptr() + 2) == api.E_INVALIDARG
        assert call(ys[2].data_ptr() + 8) == api.E_INVALIDARG                                   # rows start inside a Y plane
        assert call(uvs[4].data_ptr() - (n * BINS * 4 - 4)) == api.E_INVALIDARG                # the last word of the rows lies on a UV plane
        vp.Synchronize()
        assert torch.equal(rows, keep_rows) and all(torch.equal(a, b) for a, b in zip(ys + uvs, keep_y + keep_uv)), (own, "a refused call wrote")
        # the plain call afterwards reports its old launch count
        vp.ProcessBatchYuv(frames, NV12, desc, ys, pitch, uvs, pitch)
        vp.Synchronize()
        assert vp.GetLastBatchInfo()["launches"] == plain["launches"], (own, vp.GetLastBatchInfo(), plain)
        assert torch.equal(rows, keep_rows)
        vp.close()
    assert np.array_equal(results[False], results[True])
    ref.close()
