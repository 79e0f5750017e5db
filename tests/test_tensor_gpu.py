"""k_tensor (extension: rendered frames as float tensors, include/mpcvr.h) on the GPU: every instantiation word for word against the numpy
model (tests/tensor_model.py) at the shapes where the kernel takes another path, every alignment of source and tensor inside a patterned
buffer whose every other byte must survive, the rounding rows of tests/test_tensor.py through the kernel, planes and rows more than 4 GiB
apart, the refusals, and mpcvr_render_tensor against a plain render + mpcvr_tensor_pass.  Everything is bits: no tolerance anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import tensor_model as TM
from tests.golden.cases import HDR10, M709, case_frame, ext
from tests.test_measure_gpu import device_words
from tests.test_parity_gpu import make_vp
from tests.test_tensor import FACTORS, IMAGENET_MEAN, IMAGENET_STD

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = TM.BGRA8, TM.RGB10A2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = tuple(1 / (255 * s) for s in IMAGENET_STD)          # three different factors: a channel that takes another's shows
BIAS = tuple(-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD))
DTYPE_NAME = {TM.F32: "f32", TM.F16: "f16", TM.BF16: "bf16"}
INSTANTIATIONS = [(f, d, l) for f in (BGRA8, RGB10A2) for d in (TM.F32, TM.F16, TM.BF16) for l in (TM.PLANAR, TM.INTERLEAVED)]
INSTANTIATION_IDS = ["%s-%s-%s" % ("rgb10" if f else "bgra8", DTYPE_NAME[d], "hwc" if l else "chw") for f, d, l in INSTANTIATIONS]


def tile():
    """(columns one wavefront covers per step, columns of a workgroup, rows of a workgroup), the constants vp_tensor.h exports"""
    text = open(os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_tensor.h")).read()
    v = {k: int(n) for k, n in re.findall(r"constexpr int (kTensor\w+) = (\d+);", text)}
    assert re.search(r"kTensorGroupCols = kTensorWaveCols;", text) and re.search(r"kTensorGroupRows = kTensorWaves \* kTensorWaveRows;", text)
    return v["kTensorWaveCols"], v["kTensorWaveCols"], v["kTensorWaves"] * v["kTensorWaveRows"]


WAVE_COLS, GROUP_COLS, GROUP_ROWS = tile()
WIDTHS = sorted({1, 2, 3, 4, 5, 7, 8, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, GROUP_COLS + 1})
HEIGHTS = (1, 2, GROUP_ROWS + 1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_noise = {}


def noise(src_fmt):
    """(max height, max width) uint32 of noise in all 32 bits (the A / X bits are random) in which every code of every channel occurs: the
    first 1024 (256) texels hold a permutation of the codes per channel.  Smaller surfaces are its top-left corner."""
    if src_fmt not in _noise:
        h, w = max(HEIGHTS), max(WIDTHS) + 2
        rng = np.random.default_rng(500 + src_fmt)
        s = rng.integers(0, 2 ** 32, size=h * w, dtype=np.uint64).astype(np.uint32)
        n, bits = (1024, 10) if src_fmt == RGB10A2 else (256, 8)
        assert s.size >= n
        r, g, b = (rng.permutation(n).astype(np.uint32) for _ in range(3))
        keep = np.uint32(0xc0000000 if src_fmt == RGB10A2 else 0xff000000)
        s[:n] = (s[:n] & keep) | ((r | g << 10 | b << 20) if src_fmt == RGB10A2 else (b | g << 8 | r << 16))
        s = s.reshape(h, w)
        c = TM.codes(s, src_fmt)
        assert all(np.unique(c[k]).size == n for k in range(3))
        _noise[src_fmt] = s
    return _noise[src_fmt]


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 17) & 255).astype(np.uint8)


def run_pass(torch, words, src_fmt, dtype, layout, order, scale=SCALE, bias=BIAS, src_off=0, src_pitch=None, dst_off=0, row_pitch=None, plane_pad=0):
    """One mpcvr_tensor_pass of `words` ((h, w) uint32) from a source src_off bytes behind a 256-byte boundary into a tensor dst_off bytes
    behind one, inside a patterned buffer with a guard of one row pitch + 4 KiB in front and behind.  Asserts the WHOLE buffer: the tensor's
    elements equal the model's bits, every other byte (pitch padding, gaps between planes, guards) holds the pattern."""
    from videorenderer_amd import api
    h, w = words.shape
    es = TM.ELEMENT_SIZE[dtype]
    src_pitch = src_pitch or 4 * w
    row_pitch = row_pitch or es * w * (1 if layout == TM.PLANAR else 3)
    plane_pitch = row_pitch * h + plane_pad if layout == TM.PLANAR else 0
    host = np.full(256 + src_off + h * src_pitch, 0xa5, dtype=np.uint8)
    for y in range(h):
        host[256 + src_off + y * src_pitch:][:4 * w] = words[y].view(np.uint8)
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 256 == 0
    guard = (row_pitch + 4096 + 255) // 256 * 256
    extent = (3 * plane_pitch if layout == TM.PLANAR else h * row_pitch)
    total = guard + dst_off + extent + guard
    before = pattern(total)
    buf = torch.from_numpy(before).cuda()
    assert buf.data_ptr() % 256 == 0
    d = api.tensor_desc(dtype, layout, row_pitch, plane_pitch, scale, bias, order)
    api.tensor_pass(src.data_ptr() + 256 + src_off, src_pitch, src_fmt, w, h, d, buf.data_ptr() + guard + dst_off)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = TM.place(before.copy(), guard + dst_off, TM.tensor(words, src_fmt, dtype, layout, order, scale, bias), layout, row_pitch, plane_pitch)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        off = int(bad[0]) - guard - dst_off
        raise AssertionError("%dx%d %s dtype %d layout %d order %d, source +%d pitch %d, tensor +%d row pitch %d plane pitch %d: %d bytes differ, the first "
                             "%d bytes from the tensor's first (got %#x, want %#x, pattern %#x)"
                             % (w, h, "rgb10" if src_fmt else "bgra8", dtype, layout, order, src_off, src_pitch, dst_off, row_pitch, plane_pitch, bad.size, off,
                                got[bad[0]], want[bad[0]], before[bad[0]]))
    assert src.cpu().numpy().tobytes() == host.tobytes()


@pytest.mark.parametrize("src_fmt,dtype,layout", INSTANTIATIONS, ids=INSTANTIATION_IDS)
def test_every_instantiation_equals_the_model_word_for_word(mpcvr, torch_cuda, src_fmt, dtype, layout):
    """every width and height at which a lane, a wavefront or a workgroup begins or ends, both channel orders, tight source and tensor"""
    full = noise(src_fmt)
    for h in HEIGHTS:
        for w in WIDTHS:
            words = np.ascontiguousarray(full[:h, :w])
            for order in (TM.RGB, TM.BGR):
                run_pass(torch_cuda, words, src_fmt, dtype, layout, order)


@pytest.mark.parametrize("src_fmt,dtype,layout", INSTANTIATIONS, ids=INSTANTIATION_IDS)
def test_alignments_and_pitches_leave_every_other_byte_alone(mpcvr, torch_cuda, src_fmt, dtype, layout):
    """Source at +0 / +4 / +8 off a 16-byte boundary with a pitch that is and is not a multiple of 16 (the 16-byte loads step aside), tensor at
    +0 / +es / +8 off 16 with rows tight, padded to 16 + 64 and padded by ONE element (the vector stores step aside): the same elements, and
    the pattern around them survives.  13 columns: three full lanes and a tail; 259: a second wavefront piece of three columns."""
    es = TM.ELEMENT_SIZE[dtype]
    full = noise(src_fmt)
    per = es * (1 if layout == TM.PLANAR else 3)
    n = 0
    for w, h in ((13, 3), (WAVE_COLS + 3, 2)):
        words = np.ascontiguousarray(full[:h, :w])
        tight = per * w
        for src_off in (0, 4, 8):
            for src_pitch in ((4 * w + 15) // 16 * 16 + 16, (4 * w + 15) // 16 * 16 + 4):
                for dst_off in (0, es, 8):
                    for row_pitch, plane_pad in ((tight, 0), ((tight + 15) // 16 * 16 + 64, 0), (tight + es, 0), ((tight + 15) // 16 * 16, es)):
                        run_pass(torch_cuda, words, src_fmt, dtype, layout, (n >> 1) & 1, src_off=src_off, src_pitch=src_pitch, dst_off=dst_off,
                                 row_pitch=row_pitch, plane_pad=plane_pad if layout == TM.PLANAR else 0)
                        n += 1


@pytest.mark.parametrize("dtype", [TM.F32, TM.F16, TM.BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("src_fmt", [BGRA8, RGB10A2], ids=["bgra8", "rgb10"])
def test_the_rounding_rows_through_the_kernel(mpcvr, torch_cuda, src_fmt, dtype):
    """the (scale, bias) table of tests/test_tensor.py over all codes: ties, overflow to inf, fp16 subnormals, negative scales, cancelling
    biases — three rows at a time, one per channel, so each row meets every code"""
    n = 1024 if src_fmt == RGB10A2 else 256
    c = np.arange(n, dtype=np.uint32)
    words = ((c | c << 10 | c << 20 | np.uint32(0x80000000)) if src_fmt == RGB10A2 else (c | c << 8 | c << 16 | np.uint32(0x7f000000))).reshape(n // 32, 32)
    rows = list(FACTORS.values())
    rows += rows[: -len(rows) % 3]
    for i in range(0, len(rows), 3):
        scale, bias = zip(*rows[i:i + 3])
        for layout in (TM.PLANAR, TM.INTERLEAVED):
            run_pass(torch_cuda, words, src_fmt, dtype, layout, TM.RGB, scale=scale, bias=bias)


# ---- planes and rows more than 4 GiB apart ------------------------------------------------------------------------------------------------
FAR = (1 << 32) + 4096
FAR_GUARD = 1 << 16                        # patterned bytes in front of and behind every written row


@pytest.fixture(scope="module")
def far_buffer(torch_cuda):
    """one allocation for the module: three places FAR apart with a guard around each (8 GiB + 192 KiB; the suite's huge-layout tests hold
    to 10 GiB).  Only the neighbourhoods of written rows are ever filled or read."""
    torch = torch_cuda
    torch.cuda.empty_cache()
    buf = torch.empty(2 * FAR + 3 * FAR_GUARD, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


def far_check(torch, buf, words, src_fmt, dtype, layout, row_pitch, plane_pitch):
    """The pass into buf + FAR_GUARD with the given pitches; every written row is read back with FAR_GUARD / 2 bytes in front and behind,
    which must hold the pattern they were given (rows of a 64-column frame are at most 768 bytes)."""
    from videorenderer_amd import api
    h, w = words.shape
    es = TM.ELEMENT_SIZE[dtype]
    bits = TM.tensor(words, src_fmt, dtype, layout, TM.BGR, SCALE, BIAS)
    half = FAR_GUARD // 2
    rows = [(k * plane_pitch + y * row_pitch, bits[k, y]) for k in range(3) for y in range(h)] if layout == TM.PLANAR else \
           [(y * row_pitch, bits[y].reshape(-1)) for y in range(h)]
    starts = sorted({(FAR_GUARD + off - half) for off, _ in rows})
    windows = []
    for s in starts:                       # the windows of neighbouring rows may overlap (planes of small pitch): fill each stretch once
        if windows and s < windows[-1][1]:
            windows[-1][1] = s + FAR_GUARD
        else:
            windows.append([s, s + FAR_GUARD])
    for a, b in windows:
        assert 0 <= a and b <= buf.numel()
        buf[a:b] = torch.from_numpy(pattern(b - a)).cuda()
    src = torch.from_numpy(words.view(np.int32)).cuda()
    d = api.tensor_desc(dtype, layout, row_pitch, plane_pitch, SCALE, BIAS, TM.BGR)
    api.tensor_pass(src, 4 * w, src_fmt, w, h, d, buf.data_ptr() + FAR_GUARD)
    torch.cuda.synchronize()
    for a, b in windows:
        got = buf[a:b].cpu().numpy()
        want = pattern(b - a)
        for off, row in rows:
            at = FAR_GUARD + off - a
            if 0 <= at < b - a:
                want[at:at + row.size * es] = row.view(np.uint8)
        assert np.array_equal(got, want), ("bytes %d .. %d of the buffer" % (a, b), np.nonzero(got != want)[0][:8])


@pytest.mark.parametrize("src_fmt,dtype", [(BGRA8, TM.F16), (RGB10A2, TM.F32), (BGRA8, TM.BF16)], ids=["bgra8-f16", "rgb10-f32", "bgra8-bf16"])
def test_planes_more_than_4_gib_apart(mpcvr, torch_cuda, far_buffer, src_fmt, dtype):
    """64 x 32, C,H,W, the three planes 2^32 + 4096 bytes apart: a plane offset kept in 32 bits lands in the first plane's neighbourhood"""
    words = np.ascontiguousarray(noise(src_fmt)[:GROUP_ROWS + 1, :64])
    words = np.concatenate([words] * 4)[:32]
    far_check(torch_cuda, far_buffer, words, src_fmt, dtype, TM.PLANAR, 64 * TM.ELEMENT_SIZE[dtype] + 64, FAR)


@pytest.mark.parametrize("src_fmt,dtype,layout", [(BGRA8, TM.F16, TM.INTERLEAVED), (RGB10A2, TM.F32, TM.INTERLEAVED), (RGB10A2, TM.BF16, TM.INTERLEAVED)],
                         ids=["bgra8-f16-hwc", "rgb10-f32-hwc", "rgb10-bf16-hwc"])
def test_rows_more_than_4_gib_apart(mpcvr, torch_cuda, far_buffer, src_fmt, dtype, layout):
    """Rows 2^32 + 4096 bytes apart.  Three rows of 64 columns: the second row of a wavefront and the first of the next — 32 rows that far
    apart would take 124 GiB, and a C,H,W tensor with such rows three times that, where the suite's huge-layout tests hold to 10 GiB; a row
    offset kept in 32 bits shows at the second row already, in the first row's neighbourhood."""
    words = np.ascontiguousarray(noise(src_fmt)[:3, :64])
    far_check(torch_cuda, far_buffer, words, src_fmt, dtype, layout, FAR, 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h = 16, 8
    src = torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda")
    before = pattern(1 << 14)
    buf = torch.from_numpy(before).cuda()
    s0, d0 = src.data_ptr(), buf.data_ptr() + 4096

    def call(w=w, h=h, s=s0, sp=w * 4, fmt=BGRA8, dst=d0, desc=True, **kw):
        es = TM.ELEMENT_SIZE.get(kw.get("dtype", TM.F32), 4)
        lay = kw.get("layout", TM.PLANAR)
        rp = kw.pop("row_pitch", es * 16 * (1 if lay == TM.PLANAR else 3))
        d = api.tensor_desc(kw.get("dtype", TM.F32), lay, rp, kw.pop("plane_pitch", rp * 8), kw.get("scale", SCALE), kw.get("bias", BIAS), kw.get("order", TM.RGB))
        d.reserved = kw.get("reserved", 0)
        return L.mpcvr_tensor_pass(C.c_void_p(s), sp, fmt, w, h, C.byref(d) if desc else None, C.c_void_p(dst), None)

    E = api.E_INVALIDARG
    for kw, hr in ((dict(s=None), api.E_POINTER), (dict(dst=None), api.E_POINTER), (dict(desc=False), api.E_POINTER),
                   (dict(fmt=2), E), (dict(w=0), E), (dict(h=0), E), (dict(w=32769), E), (dict(h=32769), E), (dict(sp=60), E), (dict(sp=66), E), (dict(s=s0 + 2), E),
                   (dict(dtype=3), E), (dict(layout=2), E), (dict(order=2), E), (dict(reserved=7), E),
                   (dict(scale=(1.0, float("inf"), 1.0)), E), (dict(scale=(float("nan"), 1.0, 1.0)), E), (dict(scale=(1.0, 1.0, 2.0 ** 101)), E),
                   (dict(scale=(2.0 ** -101, 1.0, 1.0)), E), (dict(bias=(0.0, float("nan"), 0.0)), E), (dict(bias=(0.0, 0.0, -(2.0 ** 101))), E),
                   (dict(bias=(float("inf"), 0.0, 0.0)), E), (dict(bias=(2.0 ** -101, 0.0, 0.0)), E),
                   (dict(row_pitch=60), E), (dict(row_pitch=0), E), (dict(row_pitch=-64), E), (dict(row_pitch=66), E), (dict(row_pitch=(1 << 47) + 4), E),
                   (dict(layout=TM.INTERLEAVED, row_pitch=188), E), (dict(plane_pitch=0), E), (dict(plane_pitch=-512), E), (dict(plane_pitch=514), E),
                   (dict(plane_pitch=(1 << 47) + 4), E), (dict(dst=d0 + 2), E), (dict(dtype=TM.F16, dst=d0 + 1), E), (dict(dtype=TM.BF16, row_pitch=33), E),
                   (dict(plane_pitch=64 * 7 + 60), E),               # the second plane starts in the first one's last row
                   (dict(row_pitch=192, plane_pitch=64), E),       # planes that interleave row by row
                   (dict(dst=s0), E), (dict(dst=s0 - 3 * 512 + 4), E), (dict(layout=TM.INTERLEAVED, dst=s0 + 508), E)):      # over the source
        assert call(**kw) == hr, kw
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before) and not bool(src.any())
    assert call() == 0          # ... and the arguments they were derived from are accepted
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = TM.place(before.copy(), 4096, TM.tensor(np.zeros((h, w), np.uint32), BGRA8, TM.F32, TM.PLANAR, TM.RGB, SCALE, BIAS), TM.PLANAR, 64, 512)
    assert np.array_equal(got, want)


# ---- mpcvr_render_tensor ------------------------------------------------------------------------------------------------------------------
RENDER_CASES = {
    "sdr_8bit": dict(cformat=1, w=96, h=64, kind="structure", seed=171, exfmt=ext(matrix=M709), iUpscaling=2, dst=(96, 64)),
    "hdr10_rgb10a2": dict(cformat=2, w=96, h=64, kind="hdr", seed=172, exfmt=HDR10, iUpscaling=4, output_format=1, hdr_output=1, dst=(192, 128)),
    "letterboxed_odd_window": dict(cformat=1, w=96, h=64, kind="structure", seed=173, exfmt=ext(matrix=M709), iUpscaling=2, dst=(77, 57), window=(95, 63), offset=(9, 3)),
}


def rendered(mpcvr, torch, c):
    vp, (ww, wh) = make_vp(mpcvr, c)
    frame, pitch = case_frame(c)
    dev = torch.from_numpy(frame).cuda()
    vp.CopySample(dev, pitch)
    return vp, dev, ww, wh


def bits_of(t):
    """a float tensor's elements as unsigned words on the host"""
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint16)


@pytest.mark.parametrize("label", list(RENDER_CASES))
def test_render_tensor_equals_render_then_tensor_pass(mpcvr, torch_cuda, label):
    from videorenderer_amd import api
    torch = torch_cuda
    c = RENDER_CASES[label]
    fmt = c.get("output_format", 0)
    vp, keep, ww, wh = rendered(mpcvr, torch, c)
    # a plain render on a second context: its back buffer is the reference surface
    vp2, keep2, _, _ = rendered(mpcvr, torch, c)
    assert vp2.Render(1) == 0
    vp2.Synchronize()
    ptr, pitch, w2, h2 = vp2.GetBackBuffer()
    assert (w2, h2, pitch) == (ww, wh, ww * 4)
    surface = device_words(ptr, ww * wh).reshape(wh, ww)
    shown2 = vp2.GetDisplayedImage(deep_color=True)
    for dt, layout, order in ((torch.float16, "chw", "rgb"), (torch.float32, "hwc", "bgr"), (torch.bfloat16, "chw", "bgr"), (torch.float16, "hwc", "rgb")):
        out = vp.RenderTensor(dtype=dt, layout=layout, channel_order=order, scale=SCALE, bias=BIAS)
        vp.Synchronize()
        assert out.dtype == dt and tuple(out.shape) == ((3, wh, ww) if layout == "chw" else (wh, ww, 3)) and out.is_contiguous()
        want = TM.tensor(surface, fmt, api._tensor_dtype(dt), TM.PLANAR if layout == "chw" else TM.INTERLEAVED, TM.BGR if order == "bgr" else TM.RGB, SCALE, BIAS)
        assert np.array_equal(bits_of(out), want), (label, dt, layout, order)
        # ... and through the standalone pass over the other context's back buffer
        out2 = torch.zeros_like(out)
        es = out.element_size()
        d = api.tensor_desc(api._tensor_dtype(dt), TM.PLANAR if layout == "chw" else TM.INTERLEAVED, es * ww * (1 if layout == "chw" else 3), es * ww * wh, SCALE, BIAS,
                            TM.BGR if order == "bgr" else TM.RGB)
        api.tensor_pass(ptr, pitch, fmt, ww, wh, d, out2)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.uint8), out2.view(torch.uint8))
        # the frame afterwards is what GetDisplayedImage shows, and what a plain render leaves
        shown = vp.GetDisplayedImage(deep_color=True)
        assert shown[1:] == shown2[1:] and np.array_equal(shown[0], shown2[0])
        assert vp.GetBackBuffer()[1:] == (ww * 4, ww, wh)
    if "offset" in c:       # the letterbox is black: code 0 in every channel
        black = TM.element_bits(np.zeros(3, np.uint32), 1.0, 0.0, TM.F16)
        out = vp.RenderTensor(scale=(1.0,) * 3)
        vp.Synchronize()
        o = bits_of(out)
        assert (o[:, :3] == black[0]).all() and (o[:, :, :9] == black[0]).all() and (o[:, 60:] == black[0]).all() and (o[:, :, 86:] == black[0]).all()
        assert (o[:, 3:60, 9:86] != black[0]).any()
    # into a caller's tensor with padded rows; refusals are answered before anything is drawn
    big = torch.full((3, wh + 1, ww + 5), -2.0, dtype=torch.float16, device="cuda")
    view = big[:, :wh, :ww]
    assert vp.RenderTensor(out=view, scale=SCALE, bias=BIAS) is view
    vp.Synchronize()
    assert np.array_equal(bits_of(view), TM.tensor(surface, fmt, TM.F16, TM.PLANAR, TM.RGB, SCALE, BIAS))
    assert bool((big[:, wh:] == -2).all()) and bool((big[:, :, ww:] == -2).all())
    before = big.clone()
    with pytest.raises(ValueError):
        vp.RenderTensor(out=big[:, :wh, :2 * ww:2])
    with pytest.raises(ValueError):
        vp.RenderTensor(out=big[:, :wh - 1, :ww])
    d = api.tensor_desc(TM.F16, TM.PLANAR, 2 * (ww + 5), 2 * (ww + 5) * (wh + 1) - 2 * (ww + 5) * 2, SCALE, BIAS)       # planes that overlap
    assert vp._L.mpcvr_render_tensor(vp._ctx, 1, C.byref(d), C.c_void_p(big.data_ptr())) == api.E_INVALIDARG
    d = api.tensor_desc(TM.F32, TM.INTERLEAVED, 12 * ww, 0, SCALE, BIAS)
    assert vp._L.mpcvr_render_tensor(vp._ctx, 1, C.byref(d), C.c_void_p(vp.GetBackBuffer()[0] + 4 * ww)) == api.E_INVALIDARG                 # over the back buffer
    assert vp._L.mpcvr_render_tensor(vp._ctx, 1, None, C.c_void_p(big.data_ptr())) == api.E_POINTER
    vp.Synchronize()
    assert torch.equal(big, before)
    assert np.array_equal(vp.GetDisplayedImage(deep_color=True)[0], shown2[0])
    vp.close()
    vp2.close()


def test_render_tensor_without_a_sample_and_on_the_lanes(mpcvr, torch_cuda):
    """S_FALSE with nothing written while there is no sample.  Then a context that owns its stream renders on its frame lanes: RenderTensor of
    sample A, then a Render of sample B into the same back buffer, then synchronise — the tensor belongs to A.  Several rounds, so that both
    lanes take both roles."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = RENDER_CASES["letterboxed_odd_window"]
    vp = api.VideoProcessor(api.default_settings(iUpscaling=c["iUpscaling"]), use_torch_stream=False)
    vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c["exfmt"])
    ww, wh = c["window"]
    vp.SetWindowRect((0, 0, ww, wh))
    vp.SetVideoRect((9, 3, 86, 60))
    outs = torch.full((8, wh, ww, 3), -3.0, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    assert vp.RenderTensor(out=outs[0], layout="hwc") is None
    vp.Synchronize()
    assert bool((outs == -3).all())
    samples = []
    for seed, kind in ((174, "structure"), (175, "noise")):
        frame, pitch = case_frame(dict(c, seed=seed, kind=kind))
        samples.append(torch.from_numpy(frame).cuda())
    torch.cuda.synchronize()
    want = []
    for s in samples:                                       # each sample's tensor on its own, everything synchronised
        vp.CopySample(s, pitch)
        assert vp.Render(1) == 0
        vp.Synchronize()
        ptr, bp, bw, bh = vp.GetBackBuffer()
        want.append(TM.tensor(device_words(ptr, bw * bh).reshape(bh, bw), BGRA8, TM.BF16, TM.INTERLEAVED, TM.RGB, SCALE, BIAS))
    assert not np.array_equal(want[0], want[1])
    for r in range(8):
        vp.CopySample(samples[r & 1], pitch)
        assert vp.RenderTensor(out=outs[r], layout="hwc", scale=SCALE, bias=BIAS) is not None
        vp.CopySample(samples[1 - (r & 1)], pitch)
        assert vp.Render(1) == 0
    vp.Synchronize()
    for r in range(8):
        assert np.array_equal(bits_of(outs[r]), want[r & 1]), "round %d: the tensor is not the frame's that was rendered in front of it" % r
    vp.close()
