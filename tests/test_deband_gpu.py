"""k_deband (extension: debanding of rendered frames, include/mpcvr.h) on the GPU: every instantiation texel for texel against the numpy
model (tests/deband_model.py) at the shapes where the kernel takes another path — one texel, one row, one column, the workgroup tile's
extent - 1 / 0 / + 1 and twice that + 1, a frame smaller than the halo in both directions, the largest halo across two tiles — with both
tap placements, every alignment of source and destination inside a patterned buffer whose every other byte must survive, poisoned source
padding, random A / X bits, seeds, the placement override, mpcvr_render_deband, and the refusals.  Everything is bits: no tolerance
anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import deband_model as DM
from tests.test_deband import K, PAIR_IDS, PAIRS, noise, params, smooth

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = DM.BGRA8, DM.RGB10A2
TW, TH, FIT = K["kDebandTileCols"], K["kDebandTileRows"], K["kDebandLdsFitR"]
# (w, h): one texel, one column, one row, a frame inside one tile; the tile's extent - 1 / 0 / + 1 and twice that + 1 in each direction
# ... frames smaller than the halo in both directions (7 x 5 for the smallest candidate, 27 x 21 for R >= 32), and a frame two tiles wide
SHAPES = [(1, 1), (1, 67), (67, 1), (70, 40), (TW - 1, TH + 1), (TW, TH), (TW + 1, TH - 1), (2 * TW + 1, 9), (9, 2 * TH + 1), (2 * TW + 1, 2 * TH + 1),
          (7, 5), (27, 21), (2 * TW - 3, 20)]
# (range, iterations): candidates for either placement; mpcvr_plan_deband says which placement the launcher takes for each
CANDIDATES = [(2, 2), (16, 1), (4, 4), (8, 4), (32, 1), (11, 3), (16, 4), (64, 1)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("MPCVR_DEBAND_TAPS", raising=False)


def picked(place, w=70, h=40):
    """the candidates for which the launcher takes `place` (mpcvr_plan_deband, no override)"""
    from videorenderer_amd import api
    return [(r, it) for r, it in CANDIDATES if api.plan_deband(RGB10A2, params(r, it, 0, 0), w, h)[1] == place]


_src = {}


def surface(fmt):
    """(2 TH + 1, 2 TW + 1) uint32: smooth with a code or two of noise and random A / X bits, so that thresholds accept some taps and
    refuse others; made once per format.  Smaller surfaces are its top-left corner."""
    if fmt not in _src:
        _src[fmt] = smooth(fmt, 2 * TH + 1, 2 * TW + 1, 40 + fmt)
    return _src[fmt]


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 17) & 255).astype(np.uint8)


def run_pass(torch, words, src_fmt, dst_fmt, P, seed, src_off=0, src_pitch=None, dst_off=0, dst_pitch=None, want=None, poison=None):
    """One mpcvr_deband_pass of `words` ((h, w) uint32) from a source src_off bytes behind a 256-byte boundary into a destination dst_off
    bytes behind one, each inside a patterned (source: or poisoned) buffer with a guard of one pitch + 4 KiB in front and behind.  Asserts
    the WHOLE destination buffer: the texels equal the model's, every other byte (pitch padding, guards) holds the pattern; the source is
    as it was.  Returns the texels."""
    from videorenderer_amd import api
    h, w = words.shape
    src_pitch, dst_pitch = src_pitch or 4 * w, dst_pitch or 4 * w
    sguard = (src_pitch + 4096 + 255) // 256 * 256
    n = sguard + src_off + h * src_pitch + sguard
    shost = DM.place(pattern(n) if poison is None else np.full(n, poison, dtype=np.uint8), sguard + src_off, words, src_pitch)
    src = torch.from_numpy(shost).cuda()
    guard = (dst_pitch + 4096 + 255) // 256 * 256
    before = pattern(guard + dst_off + h * dst_pitch + guard)
    buf, at = torch.from_numpy(before).cuda(), guard + dst_off
    assert src.data_ptr() % 256 == 0 and buf.data_ptr() % 256 == 0
    api.deband_pass(src.data_ptr() + sguard + src_off, src_pitch, src_fmt, w, h, P, seed, buf.data_ptr() + at, dst_pitch, dst_fmt)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    if want is None:
        want = DM.apply(words, src_fmt, dst_fmt, P["range"], P["iterations"], P["threshold"], P["dither"], seed)
    full = DM.place(before.copy(), at, want, dst_pitch)
    if not np.array_equal(got, full):
        bad = np.nonzero(got != full)[0]
        off = int(bad[0]) - at
        raise AssertionError("%dx%d %s -> %s %r seed %d (%s), source +%d pitch %d, destination +%d pitch %d: %d bytes differ, the first %d bytes from "
                             "the destination's first = row %d column %d (got %#x, want %#x, pattern %#x)"
                             % (w, h, "rgb10" if src_fmt else "bgra8", "rgb10" if dst_fmt else "bgra8", P, seed, api.plan_deband(src_fmt, P, w, h)[1], src_off,
                                src_pitch, dst_off, dst_pitch, bad.size, off, off // dst_pitch, off % dst_pitch // 4, got[bad[0]], full[bad[0]], before[bad[0]]))
    assert src.cpu().numpy().tobytes() == shost.tobytes()
    return want


@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("place", ["lds", "global"])
def test_every_instantiation_equals_the_model_texel_for_texel(mpcvr, torch_cuda, place, src_fmt, dst_fmt):
    """k_deband<IN10, OUT10, PLACE> as the test's id names it, at parameters for which the dispatcher's own rule takes PLACE, over every
    shape, tight source and destination.  R = 64 (global) and the largest halo LDS takes run on frames two tiles wide, where halos cross
    tiles, and on frames smaller than the halo in both directions, where every tap clamps."""
    from videorenderer_amd import api
    cases = picked(place)
    assert cases, "the rule never selects %s: that placement should not be in the build" % place
    full = surface(src_fmt)
    th = 24 if src_fmt else 8
    for r, it in cases:
        P = params(r, it, th, (r + it) & 1)
        for w, h in SHAPES:
            assert api.plan_deband(src_fmt, P, w, h) == (r * it, place)
            run_pass(torch_cuda, np.ascontiguousarray(full[:h, :w]), src_fmt, dst_fmt, P, 1000 + r)


@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_the_override_gives_identical_bytes(mpcvr, torch_cuda, monkeypatch, src_fmt, dst_fmt):
    """MPCVR_DEBAND_TAPS = lds | global, read per launch: both placements against the model — the same bytes — at the largest halo LDS
    takes, at a small one, and at a threshold of 0 and of 4 maxin; noise, so that nothing is smooth about the taps"""
    from videorenderer_amd import api
    words = np.ascontiguousarray(noise(src_fmt, 2 * TH + 1, 2 * TW + 1, 50 + src_fmt)[:TH + 3, :2 * TW + 1])
    h, w = words.shape
    m = DM.MAXCODE[src_fmt]
    for P in (params(FIT, 1, 4 * m, 1), params(FIT // 4, 4, 4 * m, 0), params(3, 2, 0, 1), params(1, 1, 2 * m, 1)):
        want = None
        for taps in ("lds", "global"):
            monkeypatch.setenv("MPCVR_DEBAND_TAPS", taps)
            assert api.plan_deband(src_fmt, P, w, h)[1] == taps
            want = run_pass(torch_cuda, words, src_fmt, dst_fmt, P, 77, want=want)
    # above the LDS limit the override cannot ask for LDS
    monkeypatch.setenv("MPCVR_DEBAND_TAPS", "lds")
    P = params(FIT + 1, 1, 4 * m, 1)
    assert api.plan_deband(src_fmt, P, w, h)[1] == "global"
    run_pass(torch_cuda, words, src_fmt, dst_fmt, P, 78)


@pytest.mark.parametrize("taps", ["lds", "global"])
@pytest.mark.parametrize("src_fmt,dst_fmt", [(RGB10A2, BGRA8), (BGRA8, RGB10A2)], ids=["rgb10-to-bgra8", "bgra8-to-rgb10"])
def test_alignments_and_pitches_leave_every_other_byte_alone(mpcvr, torch_cuda, monkeypatch, src_fmt, dst_fmt, taps):
    """Source and destination at +0 / +4 / +8 behind a 256-byte boundary with pitches that are and are not multiples of 16 (the 16-byte
    loads and stores step aside independently): the same texels, and the pattern around them survives.  13 columns: three full lanes and
    a tail; TW + 3: a second tile of three columns."""
    monkeypatch.setenv("MPCVR_DEBAND_TAPS", taps)
    full = surface(src_fmt)
    P = params(5, 2, 24 if src_fmt else 8, 1)
    for w, h in ((13, 3), (TW + 3, 6)):
        words = np.ascontiguousarray(full[:h, :w])
        want = DM.apply(words, src_fmt, dst_fmt, 5, 2, P["threshold"], 1, 9)
        up = (4 * w + 15) // 16 * 16
        for src_off in (0, 4, 8):
            for src_pitch in (4 * w, up + 16, up + 4):
                for dst_off in (0, 4, 8):
                    for dst_pitch in (4 * w, up + 64, up + 4):
                        run_pass(torch_cuda, words, src_fmt, dst_fmt, P, 9, src_off=src_off, src_pitch=src_pitch, dst_off=dst_off, dst_pitch=dst_pitch, want=want)


@pytest.mark.parametrize("taps", ["lds", "global"])
def test_poisoned_source_padding_does_not_show(mpcvr, torch_cuda, monkeypatch, taps):
    """the bytes between the source's rows and around it, filled with two patterns: the same frame — a clamped tap reads the edge texel,
    never the padding.  A frame smaller than the halo, so that taps clamp on every side"""
    monkeypatch.setenv("MPCVR_DEBAND_TAPS", taps)
    words = np.ascontiguousarray(noise(RGB10A2, 40, 40, 5)[:21, :27])
    P = params(FIT, 1, 4 * 1023, 1)
    want = DM.apply(words, RGB10A2, BGRA8, FIT, 1, 4 * 1023, 1, 3)
    for poison in (0x00, 0xff):
        for off, pitch in ((0, 4 * 27 + 20), (4, 4 * 27 + 4)):
            run_pass(torch_cuda, words, RGB10A2, BGRA8, P, 3, src_off=off, src_pitch=pitch, want=want, poison=poison)


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_source_alpha_bits_do_not_matter(mpcvr, torch_cuda, src_fmt):
    full = np.ascontiguousarray(surface(src_fmt)[:40, :70])
    keep = np.uint32(0x3fffffff if src_fmt else 0x00ffffff)
    rs = np.random.default_rng(8)
    P = params(16, 2, 24 if src_fmt else 8, 1)
    want = DM.apply(full & keep, src_fmt, 1 - src_fmt, 16, 2, P["threshold"], 1, 4)
    for _ in range(2):
        a = rs.integers(0, 2 ** 32, size=full.shape, dtype=np.uint64).astype(np.uint32) & ~keep
        run_pass(torch_cuda, (full & keep) | a, src_fmt, 1 - src_fmt, P, 4, want=want)


def test_seeds(mpcvr, torch_cuda):
    """two seeds give different dithered frames; the same seed gives the same bytes twice; 0 and 0xffffffff are seeds like any other"""
    words = np.ascontiguousarray(surface(RGB10A2)[:40, :70])
    P = params(16, 2, 16, 1)
    got = {s: run_pass(torch_cuda, words, RGB10A2, BGRA8, P, s) for s in (0, 1, 0xffffffff)}
    again = run_pass(torch_cuda, words, RGB10A2, BGRA8, P, 1)
    assert np.array_equal(again, got[1])
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[0xffffffff])


@pytest.mark.parametrize("label", ["sdr_8bit", "hdr10_rgb10a2", "letterboxed_odd_window"])
def test_render_deband_equals_render_then_the_model_and_leaves_the_back_buffer(mpcvr, torch_cuda, label):
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
    frame = device_words(ptr, ww * wh).reshape(wh, ww).copy()
    for P, seed, dst_fmt in ((params(16, 2, 24 if fmt else 8, 1), 5, 1 - fmt), (params(3, 4, 4 * DM.MAXCODE[fmt], 0), 0xffffffff, fmt)):
        pitch = ww * 4 + 12
        before = pattern(wh * pitch + 512)
        buf = torch.from_numpy(before).cuda()
        assert vp.RenderDeband(P, seed, dst_fmt, out=buf.data_ptr() + 256, out_pitch=pitch) is not None
        vp.Synchronize()
        model = DM.apply(frame, fmt, dst_fmt, P["range"], P["iterations"], P["threshold"], P["dither"], seed)
        assert np.array_equal(buf.cpu().numpy(), DM.place(before.copy(), 256, model, pitch)), (label, P)
        ptr1, _, bw1, bh1 = vp.GetBackBuffer()
        assert (bw1, bh1) == (ww, wh) and np.array_equal(device_words(ptr1, ww * wh).reshape(wh, ww), frame), "the back buffer changed"
    # an allocated target with the defaults of the context's format
    out = vp.RenderDeband(seed=3)
    vp.Synchronize()
    d = api.deband_params_default(fmt)
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(wh, ww), DM.apply(frame, fmt, fmt, d.range, d.iterations, d.threshold, d.dither, 3))
    # refusals come before anything is drawn: the target over the back buffer, NULLs, a parameter, a format, a pitch
    L, E = vp._L, api.E_INVALIDARG
    ok = C.byref(api.DebandParams(16, 2, 4, 1))
    keep_buf = buf.clone()
    t = C.c_void_p(buf.data_ptr() + 256)
    assert L.mpcvr_render_deband(vp._ctx, 1, ok, 0, C.c_void_p(vp.GetBackBuffer()[0] + 4 * ww), 4 * ww, 0) == E
    assert L.mpcvr_render_deband(vp._ctx, 1, C.byref(api.DebandParams(33, 2, 4, 1)), 0, t, pitch, 0) == E
    assert L.mpcvr_render_deband(vp._ctx, 1, ok, 0, t, pitch, 2) == E
    assert L.mpcvr_render_deband(vp._ctx, 1, ok, 0, t, 4 * ww - 4, 0) == E
    assert L.mpcvr_render_deband(vp._ctx, 1, None, 0, t, pitch, 0) == api.E_POINTER
    assert L.mpcvr_render_deband(vp._ctx, 1, ok, 0, None, pitch, 0) == api.E_POINTER
    vp.Synchronize()
    assert torch.equal(buf, keep_buf)
    vp.close()


def test_render_deband_without_a_sample(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    vp = api.VideoProcessor(api.default_settings())
    vp.InitMediaType(1, 96, 64)
    vp.SetWindowRect((0, 0, 96, 64))
    vp.SetVideoRect((0, 0, 96, 64))
    out = torch.full((64, 96, 4), 7, dtype=torch.uint8, device="cuda")
    assert vp.RenderDeband(out=out) is None
    vp.Synchronize()
    assert bool((out == 7).all())
    vp.close()


def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h = 16, 8
    before = pattern(1 << 15)
    buf = torch.from_numpy(before).cuda()
    base = buf.data_ptr()
    s0, d0 = base + 4096, base + 8192

    def call(s=s0, sp=w * 4, sf=BGRA8, w=w, h=h, p=(3, 2, 8, 0), d=d0, dp=w * 4, df=RGB10A2):
        return L.mpcvr_deband_pass(C.c_void_p(s), sp, sf, w, h, C.byref(api.DebandParams(*p)) if p else None, 6, C.c_void_p(d), dp, df, None)

    E = api.E_INVALIDARG
    for kw, hr in ((dict(s=None), api.E_POINTER), (dict(p=None), api.E_POINTER), (dict(d=None), api.E_POINTER), (dict(sf=2), E), (dict(df=2), E),
                   (dict(w=0), E), (dict(h=0), E), (dict(w=32769), E), (dict(h=32769), E), (dict(sp=60), E), (dict(dp=60), E), (dict(sp=66), E),
                   (dict(dp=66), E), (dict(s=s0 + 2), E), (dict(d=d0 + 1), E),
                   (dict(p=(0, 1, 8, 0)), E), (dict(p=(65, 1, 8, 0)), E), (dict(p=(16, 5, 8, 0)), E), (dict(p=(17, 4, 8, 0)), E), (dict(p=(3, 2, 1021, 0)), E),
                   (dict(p=(3, 2, -1, 0)), E), (dict(p=(3, 2, 8, 2)), E),
                   (dict(d=s0), E), (dict(d=s0 + 4), E), (dict(d=s0 + 64), E), (dict(d=s0 - 7 * 64 - 60), E), (dict(d=s0 + 7 * 64 + 60), E)):
        assert call(**kw) == hr, kw
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before), "a refused call wrote"
    # ... and the arguments they were derived from are accepted, a destination that begins where the source ends included
    assert call() == 0 and call(d=s0 + 8 * 64) == 0
    torch.cuda.synchronize()
    words = before[4096:4096 + 4 * w * h].view(np.uint32).reshape(h, w)
    model = DM.apply(words, BGRA8, RGB10A2, 3, 2, 8, 0, 6)
    want = DM.place(DM.place(before.copy(), 8192, model, 4 * w), 4096 + 8 * 64, model, 4 * w)
    assert np.array_equal(buf.cpu().numpy(), want)
