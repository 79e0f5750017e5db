"""k_encode420 (extension: rendered frames as NV12 / P010, include/mpcvr.h) on the GPU: every instantiation byte for byte against the numpy
model (tests/encode_model.py), what is written around the planes in four layouts, the refusals, mpcvr_render_yuv against a plain render +
mpcvr_encode_pass, and the NV12 it writes fed back through the convert path.  The definition itself: tests/test_encode.py (CPU)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import encode_model as EM
from tests.golden.cases import COSITED, FULL, HDR10, M709, M2020, MPEG1, MPEG2, TV, case_frame, ext
from tests.test_parity_gpu import LAYOUTS, layout_of, make_vp

pytestmark = pytest.mark.gpu

NV12, P010 = 1, 2
BGRA8, RGB10A2 = 0, 1
SITING_FIELD = {EM.CENTRE: MPEG1, EM.LEFT: MPEG2, EM.TOPLEFT: COSITED}
SITING_NAME = {EM.CENTRE: "centre", EM.LEFT: "left", EM.TOPLEFT: "topleft"}
CLOSURE_BOUND = 2       # tests/test_encode.py: the model's NV12 decodes back to the frame within 2 codes (measured there, with the reason)


def description(out_cformat, siting):
    """the two output formats under descriptions that differ in matrix AND range"""
    return ext(SITING_FIELD[siting], TV, M709) if out_cformat == NV12 else ext(SITING_FIELD[siting], FULL, M2020)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def noise_surface(w, h, src_fmt, seed):
    """(h, w) uint32 of noise in all 32 bits (the alpha bits are set at random); the first texels are the cube corners with the alpha bits
    set, then 0xffffffff and 0 — as many as the surface holds"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2 ** 32, size=(h, w), dtype=np.uint64).astype(np.uint32)
    maxin = 1023 if src_fmt == RGB10A2 else 255
    first = [int(EM.pack_rgb(np.array(c), src_fmt, alpha=255)) for c in itertools.product((0, maxin), repeat=3)] + [0xffffffff, 0]
    flat = s.reshape(-1)
    n = min(len(first), flat.size)
    flat[:n] = np.array(first[:n], dtype=np.uint32)
    return s


# where the kernel can go wrong: one block, all halo; one lane and a half; the wavefront's 256-column boundary from both sides, a tail
# block behind it and the halo lane of the second wavefront; several wavefronts and workgroup rows (the top-left row halo across them)
SHAPES = ((2, 2), (6, 2), (254, 4), (256, 4), (258, 6), (514, 66))
_surfaces = {}


def surface_for(w, h, src_fmt):
    key = (w, h, src_fmt)
    if key not in _surfaces:
        _surfaces[key] = noise_surface(w, h, src_fmt, seed=1000 + 7 * w + h + src_fmt)
    return _surfaces[key]


def to_device(torch, surface, pitch):
    """the surface in device memory at `pitch` bytes per row (the padding holds 0xa5): (tensor, address)"""
    h, w = surface.shape
    host = np.full((h, pitch), 0xa5, dtype=np.uint8)
    host[:, :w * 4] = surface.view(np.uint8).reshape(h, w * 4)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr()


def plane_arrays(torch, y, uv, out10):
    a, b = y.cpu().numpy(), uv.cpu().numpy()
    return (a.view(np.uint16), b.view(np.uint16)) if out10 else (a, b)


INSTANTIATIONS = [(s, o, k) for s in (BGRA8, RGB10A2) for o in (NV12, P010) for k in (EM.CENTRE, EM.LEFT, EM.TOPLEFT)]


@pytest.mark.parametrize("src_fmt,out_cformat,siting", INSTANTIATIONS,
                         ids=["%s-to-%s-%s" % ("rgb10" if s else "bgra8", "p010" if o == P010 else "nv12", SITING_NAME[k]) for s, o, k in INSTANTIATIONS])
def test_every_instantiation_equals_the_model_byte_for_byte(mpcvr, torch_cuda, src_fmt, out_cformat, siting):
    from videorenderer_amd import api
    torch = torch_cuda
    out10 = out_cformat == P010
    desc = description(out_cformat, siting)
    plan = api.plan_encode(out_cformat, src_fmt, desc)
    assert plan["siting"] == siting
    for w, h in SHAPES:
        surface = surface_for(w, h, src_fmt)
        want_y, want_uv = EM.encode420(surface, src_fmt, out10, plan["coef"], plan["off"], plan["shift"], siting)
        # a tight source (dword loads unless w * 4 is a multiple of 16) and one whose pitch is: the 16-byte loads, with their tail lanes
        for src_pitch in (w * 4, ((w * 4 + 15) & ~15) + 16):
            src, src_ptr = to_device(torch, surface, src_pitch)
            dt = torch.int16 if out10 else torch.uint8
            y = torch.zeros((h, w), dtype=dt, device="cuda")
            uv = torch.zeros((h // 2, w), dtype=dt, device="cuda")
            row = w * (2 if out10 else 1)
            if row % 4:        # (NV12 rows of w = 2 (mod 4) bytes: the smallest legal pitch is the next multiple of 4)
                row += 2
                y = torch.zeros((h, row), dtype=dt, device="cuda")
                uv = torch.zeros((h // 2, row), dtype=dt, device="cuda")
            api.encode_pass(src_ptr, src_pitch, src_fmt, w, h, out_cformat, desc, y, row, uv, row)
            torch.cuda.synchronize()
            got_y, got_uv = plane_arrays(torch, y, uv, out10)
            what = "%dx%d source pitch %d" % (w, h, src_pitch)
            assert np.array_equal(got_y[:, :w], want_y), (what, "Y", np.argwhere(got_y[:, :w] != want_y)[:4])
            assert np.array_equal(got_uv[:, :w], want_uv), (what, "UV", np.argwhere(got_uv[:, :w] != want_uv)[:4])
            assert not got_y[:, w:].any() and not got_uv[:, w:].any(), (what, "pitch padding written")


# ---- plane layouts ---------------------------------------------------------------------------------------------------------------------
class CarvedPlane:
    """rows x row_bytes of a plane, `pitch` bytes apart, inside a patterned device buffer: the first byte `base` bytes behind a 256-byte
    boundary, a guard of one pitch + 4 KiB in front and behind.  Plane bytes start as 0."""

    def __init__(self, torch, rows, row_bytes, pitch, base):
        self.torch, self.rows, self.row_bytes, self.pitch = torch, rows, row_bytes, pitch
        guard = pitch + 4096
        self.start = (guard + 255) // 256 * 256 + base
        total = self.start + rows * pitch + guard
        i = torch.arange(total, dtype=torch.int32, device="cuda")
        self.pattern = ((i * 131 + 17) & 255).to(torch.uint8)
        self.buf = self.pattern.clone()
        assert self.buf.data_ptr() % 256 == 0
        self._pixels(self.buf).zero_()
        self.ptr = self.buf.data_ptr() + self.start

    def _pixels(self, t):
        return t.as_strided((self.rows, self.row_bytes), (self.pitch, 1), self.start)

    def bytes(self):
        return self._pixels(self.buf).contiguous().cpu().numpy()

    def assert_guards_intact(self, what):
        rest = self.buf.clone()
        self._pixels(rest).copy_(self._pixels(self.pattern))
        if not self.torch.equal(rest, self.pattern):
            off = int(self.torch.nonzero(rest != self.pattern)[0]) - self.start
            raise AssertionError("%s: a byte outside the plane's pixels was written, %d bytes from its first (row %d, byte %d; rows are %d "
                                 "bytes of %d)" % (what, off, off // self.pitch, off % self.pitch, self.row_bytes, self.pitch))


@pytest.mark.parametrize("src_fmt,out_cformat", [(BGRA8, NV12), (RGB10A2, P010), (BGRA8, P010)], ids=["nv12", "p010", "p010_from_bgra8"])
def test_plane_layouts_leave_every_other_byte_alone(mpcvr, torch_cuda, src_fmt, out_cformat):
    """258 x 6 (a tail block behind the wavefront boundary) into planes laid out four ways — tight, pitch-padded, first byte at +4 and at +8
    from a 256-byte boundary: the same planes, and the pattern around them survives.  +4 grants dword alignment only (P010's 8-byte stores
    must step aside for two dwords), +8 all the 8-byte stores need."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h = 258, 6
    out10 = out_cformat == P010
    siting = EM.TOPLEFT
    desc = description(out_cformat, siting)
    plan = api.plan_encode(out_cformat, src_fmt, desc)
    surface = surface_for(w, h, src_fmt)
    want_y, want_uv = EM.encode420(surface, src_fmt, out10, plan["coef"], plan["off"], plan["shift"], siting)
    src, src_ptr = to_device(torch, surface, w * 4)
    row = w * (2 if out10 else 1)
    outs = {}
    for layout in LAYOUTS:
        base, pitch = layout_of(layout, (row + 3) // 4)
        assert pitch % 4 == 0 and pitch >= row and base % 4 == 0
        y = CarvedPlane(torch, h, row, pitch, base)
        uv = CarvedPlane(torch, h // 2, row, pitch, base)
        api.encode_pass(src_ptr, w * 4, src_fmt, w, h, out_cformat, desc, y.ptr, pitch, uv.ptr, pitch)
        torch.cuda.synchronize()
        what = "layout %s (first byte at +%d, pitch %d)" % (layout, base, pitch)
        y.assert_guards_intact(what + " Y")
        uv.assert_guards_intact(what + " UV")
        outs[layout] = (y.bytes(), uv.bytes())
    view = (lambda a: a.view(np.uint16)) if out10 else (lambda a: a)
    assert np.array_equal(view(outs["tight"][0]), want_y) and np.array_equal(view(outs["tight"][1]), want_uv)
    for layout in LAYOUTS[1:]:
        assert np.array_equal(outs[layout][0], outs["tight"][0]) and np.array_equal(outs[layout][1], outs["tight"][1]), layout


def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h = 16, 8
    src = torch.zeros((h, w * 4), dtype=torch.uint8, device="cuda")
    buf = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda")
    y0, uv0 = buf.data_ptr(), buf.data_ptr() + 2048
    desc = description(NV12, EM.LEFT)

    def call(w=w, h=h, y=y0, yp=w, uv=uv0, uvp=w, s=src.data_ptr(), sp=w * 4, cf=NV12):
        return L.mpcvr_encode_pass(C.c_void_p(s), sp, BGRA8, w, h, cf, desc, C.c_void_p(y), yp, C.c_void_p(uv), uvp, None)

    E = api.E_INVALIDARG
    for kw, hr in ((dict(w=15), E), (dict(h=7), E), (dict(y=y0 + 2), E), (dict(uv=uv0 + 1), E), (dict(yp=w + 2), E), (dict(uvp=w + 6), E),
                   (dict(s=src.data_ptr() + 2), E), (dict(sp=w * 4 + 2), E),
                   (dict(uv=y0 + w * (h - 1)), E),                   # UV starts in Y's last row
                   (dict(uv=y0, y=y0 + w * 2), E),                  # Y starts inside UV
                   (dict(y=src.data_ptr()), E),                     # Y over the source
                   (dict(cf=30), E), (dict(y=None), api.E_POINTER), (dict(uv=None), api.E_POINTER), (dict(s=None), api.E_POINTER)):
        assert call(**kw) == hr, kw
    torch.cuda.synchronize()
    assert bool((buf == 0x5a).all()) and not bool(src.any())
    assert call() == 0          # ... and the arguments they were derived from are accepted
    torch.cuda.synchronize()
    assert bool((buf[:w * h] == 16).all()) and bool((buf[2048:2048 + w * h // 2] == 128).all())       # black, BT.709 limited range


# ---- mpcvr_render_yuv --------------------------------------------------------------------------------------------------------------------
LETTERBOX = dict(dst=(80, 60), window=(96, 64), offset=(8, 2))
RENDER_CASES = {
    "nv12_sdr_to_nv12": (dict(cformat=1, w=96, h=64, kind="structure", seed=71, exfmt=ext(matrix=M709), iUpscaling=2, **LETTERBOX),
                         NV12, ext(MPEG2, TV, M709), 16, 128),
    "p010_pq_hdr_output_to_p010": (dict(cformat=2, w=96, h=64, kind="hdr", seed=72, exfmt=HDR10, iUpscaling=4, output_format=1, hdr_output=1, **LETTERBOX),
                                   P010, ext(MPEG2, TV, M2020), 64 << 6, 512 << 6),
}


def rendered(mpcvr, torch, c):
    vp, (ww, wh) = make_vp(mpcvr, c)
    frame, pitch = case_frame(c)
    dev = torch.from_numpy(frame).cuda()
    vp.CopySample(dev, pitch)
    return vp, dev, ww, wh


@pytest.mark.parametrize("label", list(RENDER_CASES))
def test_render_yuv_equals_render_then_encode_pass(mpcvr, torch_cuda, label):
    from videorenderer_amd import api
    torch = torch_cuda
    c, out_cformat, desc, black_y, black_c = RENDER_CASES[label]
    out10 = out_cformat == P010
    vp, keep, ww, wh = rendered(mpcvr, torch, c)
    y, uv = vp.RenderYuv(out_cformat, desc)
    vp.Synchronize()
    assert y.dtype == (torch.int16 if out10 else torch.uint8) and tuple(y.shape) == (wh, ww) and tuple(uv.shape) == (wh // 2, ww)
    got_y, got_uv = plane_arrays(torch, y, uv, out10)
    shown, sw, sh, bits = vp.GetDisplayedImage(deep_color=True)
    bptr, bpitch, bw, bh = vp.GetBackBuffer()
    assert (bw, bh, bpitch) == (ww, wh, ww * 4)
    # a plain render on a fresh context, its back buffer through the standalone pass
    vp2, keep2, _, _ = rendered(mpcvr, torch, c)
    assert vp2.Render(1) == 0
    vp2.Synchronize()
    ptr, pitch, w2, h2 = vp2.GetBackBuffer()
    assert (w2, h2, pitch) == (ww, wh, ww * 4)
    dt = torch.int16 if out10 else torch.uint8
    y2 = torch.zeros((wh, ww), dtype=dt, device="cuda")
    uv2 = torch.zeros((wh // 2, ww), dtype=dt, device="cuda")
    row = ww * (2 if out10 else 1)
    api.encode_pass(ptr, pitch, c.get("output_format", 0), ww, wh, out_cformat, desc, y2, row, uv2, row)
    torch.cuda.synchronize()
    want_y, want_uv = plane_arrays(torch, y2, uv2, out10)
    assert np.array_equal(got_y, want_y) and np.array_equal(got_uv, want_uv), label
    shown2 = vp2.GetDisplayedImage(deep_color=True)
    assert (sw, sh, bits) == shown2[1:] and np.array_equal(shown, shown2[0]), "the RGB frame behind mpcvr_render_yuv differs from a plain render's"
    # the letterbox is black: rows 0-1 and 62-63, columns 0-7 and 88-95 (left siting: the chroma block at column 88 reads column 87)
    for part in (got_y[:2], got_y[62:], got_y[:, :8], got_y[:, 88:]):
        assert (part == black_y).all(), label
    for part in (got_uv[:1], got_uv[31:], got_uv[:, :8], got_uv[:, 90:]):
        assert (part == black_c).all(), label
    assert (got_y[2:62, 8:88] != black_y).any()
    # an odd window is refused before anything is drawn: planes and back buffer untouched
    before = (y.clone(), uv.clone())
    vp.SetWindowRect((0, 0, 95, 64))
    hr = vp._L.mpcvr_render_yuv(vp._ctx, 1, out_cformat, desc, C.c_void_p(y.data_ptr()), row, C.c_void_p(uv.data_ptr()), row)
    assert hr == api.E_INVALIDARG
    vp.SetWindowRect((0, 0, 96, 63))
    assert vp._L.mpcvr_render_yuv(vp._ctx, 1, out_cformat, desc, C.c_void_p(y.data_ptr()), row, C.c_void_p(uv.data_ptr()), row) == api.E_INVALIDARG
    vp.Synchronize()
    assert torch.equal(y, before[0]) and torch.equal(uv, before[1])
    assert np.array_equal(vp.GetDisplayedImage(deep_color=True)[0], shown)
    vp.close()
    vp2.close()


def test_render_yuv_tensors_for_a_width_that_is_no_multiple_of_4(mpcvr, torch_cuda):
    """VideoProcessor.RenderYuv pads NV12 rows to the plane rule's multiple of 4 and returns (h, w) views: a 90 x 60 window against the
    standalone pass over the same context's back buffer."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = dict(cformat=1, w=96, h=64, kind="structure", seed=73, exfmt=ext(matrix=M709), iUpscaling=2, dst=(90, 60))
    desc = ext(COSITED, TV, M709)
    vp, keep, ww, wh = rendered(mpcvr, torch, c)
    y, uv = vp.RenderYuv(NV12, desc)
    vp.Synchronize()
    assert tuple(y.shape) == (60, 90) and tuple(uv.shape) == (30, 90) and y.stride(0) == 92
    ptr, pitch, _, _ = vp.GetBackBuffer()
    y2 = torch.zeros((60, 92), dtype=torch.uint8, device="cuda")
    uv2 = torch.zeros((30, 92), dtype=torch.uint8, device="cuda")
    api.encode_pass(ptr, pitch, BGRA8, 90, 60, NV12, desc, y2, 92, uv2, 92)
    torch.cuda.synchronize()
    assert torch.equal(y, y2[:, :90]) and torch.equal(uv, uv2[:, :90]) and not bool(y2[:, 90:].any()) and bool((y != 16).any())
    vp.close()


def test_nv12_from_render_yuv_decodes_back_to_the_frame_on_the_device(mpcvr, torch_cuda):
    """A same-size render of an NV12 frame that is constant over 2x2 blocks (nearest chroma: the RGB frame is, too), written as NV12 with
    centre siting, handed to a second context as a device sample: its frame equals the first context's back buffer within what the CPU
    closure measured (tests/test_encode.py: 2 codes, the quantisation of limited-range YCbCr) + 1 for the default tier's <= 1 code against
    the oracle."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h = 96, 64
    rng = np.random.default_rng(9)
    luma = np.repeat(np.repeat(rng.integers(16, 236, size=(h // 2, w // 2), dtype=np.uint8), 2, 0), 2, 1)
    chroma = rng.integers(16, 241, size=(h // 2, w), dtype=np.uint8)
    frame = np.concatenate([luma.reshape(-1), chroma.reshape(-1)])
    desc = ext(MPEG1, TV, M709)
    ctxs = []
    for _ in range(2):
        vp = api.VideoProcessor(api.default_settings(iChromaScaling=0, bUseDither=0))
        vp.InitMediaType(NV12, w, h, pitch=w, extfmt=desc)
        vp.SetWindowRect((0, 0, w, h))
        vp.SetVideoRect((0, 0, w, h))
        ctxs.append(vp)
    a, b = ctxs
    dev = torch.from_numpy(frame).cuda()
    a.CopySample(dev, w)
    sample = torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda")         # Y, then UV: one NV12 sample
    hr = a._L.mpcvr_render_yuv(a._ctx, 1, NV12, desc, C.c_void_p(sample.data_ptr()), w, C.c_void_p(sample.data_ptr() + w * h), w)
    assert hr == 0
    a.Synchronize()
    first = a.GetDisplayedImage()[0].reshape(h, w, 4)[..., :3].astype(np.int16)
    blocks = first.reshape(h // 2, 2, w // 2, 2, 3)
    assert (blocks == blocks[:, :1, :, :1]).all(), "the rendered frame is not constant over 2x2 blocks"
    b.CopySample(sample, w, api.MEM_DEVICE)
    dst = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    b.Process(dst, w * 4)
    b.Synchronize()
    second = dst.cpu().numpy()[..., :3].astype(np.int16)
    diff = np.abs(second - first)
    print("device round trip: max |difference| =", diff.max(), "codes; per channel (B, G, R)", diff.reshape(-1, 3).max(0))
    assert diff.max() <= CLOSURE_BOUND + 1
    a.close()
    b.close()
