"""k_lut3d (extension: a 3D colour LUT over rendered frames, include/mpcvr.h) on the GPU: every instantiation texel for texel against the
numpy model (tests/lut3d_model.py) at the shapes where the kernel takes another path and at table sizes on both sides of the LDS limit and
of the dispatcher's rule, every alignment of source and destination inside a patterned buffer whose every other byte must survive, in
place, a launch with a frame dimension, a surface whose last row begins beyond 4 GiB, and the refusals.  Everything is bits: no tolerance
anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import huge_layouts as HL
from tests import lut3d_model as LM
from tests.test_lut3d import PAIR_IDS, PAIRS, random_table

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = LM.BGRA8, LM.RGB10A2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 17, 27, 28, 33, 65)


def kernel_constants():
    """the constants vp_lut3d.h exports: the tile, and the dispatcher's rule"""
    text = open(os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_lut3d.h")).read()
    v = {k: int(n) for k, n in re.findall(r"constexpr int (kLut3d\w+) = (\d+);", text)}
    assert re.search(r"kLut3dGroupCols = kLut3dWaveCols;", text) and re.search(r"kLut3dGroupRows = kLut3dWaves \* kLut3dWaveRows;", text)
    return v


K = kernel_constants()
WAVE_COLS, GROUP_COLS, GROUP_ROWS = K["kLut3dWaveCols"], K["kLut3dWaveCols"], K["kLut3dWaves"] * K["kLut3dWaveRows"]
WIDTHS = sorted({1, 2, 3, 4, 5, 7, 8, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, GROUP_COLS + 1})
HEIGHTS = (1, 2, GROUP_ROWS + 1, K["kLut3dLdsWideWaves"] * K["kLut3dWaveRows"] + 1)      # (the wide workgroups of the larger LDS tables)
LDS_FIT_N = K["kLut3dLdsFitN"]
assert LDS_FIT_N ** 3 * 8 <= 160 * 1024 < (LDS_FIT_N + 1) ** 3 * 8 and LDS_FIT_N in SIZES and LDS_FIT_N + 1 in SIZES


def placement(n):
    """where the dispatcher reads a table of size n from, by the rule vp_lut3d.h states (kLut3dLdsMaxN: 0 = never from LDS)"""
    m = K.get("kLut3dLdsMaxN", 0)
    assert m <= LDS_FIT_N
    return "lds" if n <= m else "global"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_noise, _tables = {}, {}


def noise(src_fmt):
    """(max height, max width) uint32 of noise in all 32 bits (the A / X bits are random) in which every code of every channel occurs: the
    first 1024 (256) texels hold a permutation of the codes per channel.  Smaller surfaces are its top-left corner."""
    if src_fmt not in _noise:
        h, w = max(HEIGHTS), max(WIDTHS) + 2
        rng = np.random.default_rng(700 + src_fmt)
        s = rng.integers(0, 2 ** 32, size=h * w, dtype=np.uint64).astype(np.uint32)
        n = LM.MAXCODE[src_fmt] + 1
        assert s.size >= n
        r, g, b = (rng.permutation(n).astype(np.uint32) for _ in range(3))
        keep = np.uint32(0xc0000000 if src_fmt == RGB10A2 else 0xff000000)
        s[:n] = (s[:n] & keep) | ((r | g << 10 | b << 20) if src_fmt == RGB10A2 else (b | g << 8 | r << 16))
        s = s.reshape(h, w)
        c = LM.codes(s, src_fmt)
        assert all(np.unique(c[k]).size == n for k in range(3))
        _noise[src_fmt] = s
    return _noise[src_fmt]


def table(torch, n):
    """(host entries, device tensor) of a random table of size n with random pad words: made and uploaded once, never written"""
    if n not in _tables:
        host = random_table(n, 1000 + n)
        dev = torch.from_numpy(host.view(np.int16)).cuda()
        assert dev.data_ptr() % 8 == 0
        _tables[n] = (host, dev)
    return _tables[n]


_want = {}


def expected(words, src_fmt, dst_fmt, host, n, key=None):
    """the model over `words`; with a key the result is computed once and shared"""
    if key is None:
        return LM.apply(words, host, n, src_fmt, dst_fmt)
    if key not in _want:
        _want[key] = LM.apply(words, host, n, src_fmt, dst_fmt)
    return _want[key]


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 17) & 255).astype(np.uint8)


def run_pass(torch, words, src_fmt, dst_fmt, n, src_off=0, src_pitch=None, dst_off=0, dst_pitch=None, in_place=False, want=None):
    """One mpcvr_lut3d_pass of `words` ((h, w) uint32) from a source src_off bytes behind a 256-byte boundary into a destination dst_off
    bytes behind one (in_place: the source itself), each inside a patterned buffer with a guard of one pitch + 4 KiB in front and behind.
    Asserts the WHOLE destination buffer: the texels equal the model's, every other byte (pitch padding, guards) holds the pattern; the
    source and the table are as they were."""
    from videorenderer_amd import api
    h, w = words.shape
    host, dev = table(torch, n)
    src_pitch = src_pitch or 4 * w
    dst_pitch = src_pitch if in_place else (dst_pitch or 4 * w)
    sguard = (src_pitch + 4096 + 255) // 256 * 256
    shost = LM.place(pattern(sguard + src_off + h * src_pitch + sguard), sguard + src_off, words, src_pitch)
    src = torch.from_numpy(shost).cuda()
    assert src.data_ptr() % 256 == 0
    if in_place:
        buf, before, at = src, pattern(shost.size), sguard + src_off
    else:
        guard = (dst_pitch + 4096 + 255) // 256 * 256
        before = pattern(guard + dst_off + h * dst_pitch + guard)
        buf, at = torch.from_numpy(before).cuda(), guard + dst_off
        assert buf.data_ptr() % 256 == 0
    api.lut3d_pass(src.data_ptr() + sguard + src_off, src_pitch, src_fmt, w, h, dev, n, buf.data_ptr() + at, dst_pitch, dst_fmt)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    if want is None:
        want = expected(words, src_fmt, dst_fmt, host, n)
    full = LM.place(before.copy(), at, want, dst_pitch)
    if not np.array_equal(got, full):
        bad = np.nonzero(got != full)[0]
        off = int(bad[0]) - at
        raise AssertionError("%dx%d %s -> %s n %d (%s), source +%d pitch %d, destination +%d pitch %d%s: %d bytes differ, the first %d bytes from the "
                             "destination's first = row %d column %d (got %#x, want %#x, pattern %#x)"
                             % (w, h, "rgb10" if src_fmt else "bgra8", "rgb10" if dst_fmt else "bgra8", n, placement(n), src_off, src_pitch, dst_off, dst_pitch,
                                " in place" if in_place else "", bad.size, off, off // dst_pitch, off % dst_pitch // 4, got[bad[0]], full[bad[0]], before[bad[0]]))
    if not in_place:
        assert src.cpu().numpy().tobytes() == shost.tobytes()
    assert np.array_equal(dev.cpu().numpy().view(np.uint16), host)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_every_instantiation_equals_the_model_texel_for_texel(mpcvr, torch_cuda, src_fmt, dst_fmt, n):
    """every width and height at which a lane, a wavefront or a workgroup begins or ends, tight source and destination; the table sizes
    take both placements (test_the_dispatcher_places_the_table_by_its_rule reads which from the library)"""
    full = noise(src_fmt)
    host, _ = table(torch_cuda, n)
    whole = expected(full, src_fmt, dst_fmt, host, n, key=(src_fmt, dst_fmt, n))         # (a texel's result does not depend on its place)
    for h in HEIGHTS:
        for w in WIDTHS:
            run_pass(torch_cuda, np.ascontiguousarray(full[:h, :w]), src_fmt, dst_fmt, n, want=np.ascontiguousarray(whole[:h, :w]))


@pytest.mark.parametrize("n", (17, 33))
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_alignments_and_pitches_leave_every_other_byte_alone(mpcvr, torch_cuda, src_fmt, dst_fmt, n):
    """Source and destination at +0 / +4 / +8 behind a 256-byte boundary with pitches that are and are not multiples of 16 (the 16-byte
    loads and stores step aside independently): the same texels, and the pattern around them survives.  13 columns: three full lanes and
    a tail; 259: a second wavefront piece of three columns."""
    full = noise(src_fmt)
    host, _ = table(torch_cuda, n)
    whole = expected(full, src_fmt, dst_fmt, host, n, key=(src_fmt, dst_fmt, n))
    for w, h in ((13, 3), (WAVE_COLS + 3, 2)):
        words, want = np.ascontiguousarray(full[:h, :w]), np.ascontiguousarray(whole[:h, :w])
        up = (4 * w + 15) // 16 * 16
        for src_off in (0, 4, 8):
            for src_pitch in (up + 16, up + 4):
                for dst_off in (0, 4, 8):
                    for dst_pitch in (4 * w, up + 64, up + 4):
                        run_pass(torch_cuda, words, src_fmt, dst_fmt, n, src_off=src_off, src_pitch=src_pitch, dst_off=dst_off, dst_pitch=dst_pitch, want=want)


@pytest.mark.parametrize("n", (3, 27, 28, 65))
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_in_place(mpcvr, torch_cuda, src_fmt, dst_fmt, n):
    """dst == src with the same pitch: every texel is read before it is written, by the same lane — aligned and not, tight and padded,
    a tail lane, several wavefront pieces and workgroups"""
    full = noise(src_fmt)
    host, _ = table(torch_cuda, n)
    whole = expected(full, src_fmt, dst_fmt, host, n, key=(src_fmt, dst_fmt, n))
    for w, h in ((1, 1), (13, 3), (WAVE_COLS + 3, GROUP_ROWS + 1), (GROUP_COLS + 1, 2)):
        words, want = np.ascontiguousarray(full[:h, :w]), np.ascontiguousarray(whole[:h, :w])
        for off, pitch in ((0, None), (4, 4 * w + 4), (8, (4 * w + 15) // 16 * 16 + 32), (0, (4 * w + 15) // 16 * 16)):
            run_pass(torch_cuda, words, src_fmt, dst_fmt, n, src_off=off, src_pitch=pitch, in_place=True, want=want)


def batch_context(own=False, output_format=0):
    """a context that draws an exact 2x of 128 x 18 NV12-like noise at (1, 1) of a 259 x 39 window: a tail lane in a second wavefront piece,
    a short last tile in both directions, and a letterbox"""
    from tests.golden.cases import HDR10
    from tests.test_batch_tensor_gpu import context
    c = dict(cformat=2, w=128, h=18, kind="noise", seed=931, dst=(256, 36), window=(259, 39), offset=(1, 1), exfmt=HDR10, iUpscaling=4, output_format=output_format)
    return (c,) + context(c, own)


@pytest.mark.parametrize("n", (17, 33))
def test_the_frame_dimension_three_frames_with_a_short_last_tile(mpcvr, torch_cuda, n):
    """ONE launch over three frames of 259 x 39 (mpcvr_process_batch_lut3d, one chunk): each frame equals the model over the frame
    mpcvr_process_batch draws, and the bytes between the targets' rows survive"""
    from tests.test_batch_tensor_gpu import noise_frames
    torch = torch_cuda
    host, dev = table(torch, n)
    c, vp, ww, wh = batch_context(output_format=1)
    frames = noise_frames(torch, c, 3)
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    plain = vp.GetLastBatchInfo()["launches"]
    pitch = 4 * ww + 20
    before = pattern(3 * wh * pitch)
    buf = torch.from_numpy(before).cuda()
    vp.ProcessBatchLut3d(frames, dev, n, [buf.data_ptr() + i * wh * pitch for i in range(3)], pitch, BGRA8)
    vp.Synchronize()
    info = vp.GetLastBatchInfo()
    assert info["lut3d_chunks"] == 1 and info["launches"] == plain + 1 and info["lut3d_table"] == placement(n), info
    want = before.copy()
    for i, t in enumerate(rgb):
        LM.place(want, i * wh * pitch, LM.apply(t.cpu().numpy().view(np.uint32).reshape(wh, ww), host, n, RGB10A2, BGRA8), pitch)
    assert np.array_equal(buf.cpu().numpy(), want)
    vp.close()


@pytest.mark.parametrize("n", SIZES)
def test_the_dispatcher_places_the_table_by_its_rule(mpcvr, torch_cuda, n):
    """the placement the library reports (mpcvr_get_last_batch_info: lut3d_table) is the one vp_lut3d.h's rule gives, on both sides of the
    LDS limit (27 | 28) and of the rule; the frame is the model's either way"""
    from tests.test_batch_tensor_gpu import noise_frames
    torch = torch_cuda
    host, dev = table(torch, n)
    c, vp, ww, wh = batch_context()
    frames = noise_frames(torch, c, 1)
    rgb = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatch(frames, [rgb], ww * 4)
    out = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatchLut3d(frames, dev, n, [out], ww * 4, RGB10A2)
    vp.Synchronize()
    info = vp.GetLastBatchInfo()
    assert info["lut3d_table"] == placement(n), (n, info)
    if n > LDS_FIT_N:
        assert info["lut3d_table"] == "global"
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(wh, ww), LM.apply(rgb.cpu().numpy().view(np.uint32).reshape(wh, ww), host, n, BGRA8, RGB10A2))
    vp.close()


def test_a_surface_whose_last_row_begins_beyond_4_gib(mpcvr, torch_cuda):
    """3 rows of a 64-column picture at a pitch of 2^31 - 256 in one allocation (tests/huge_layouts.py: 2 GiB lead, then the surface): as
    the destination, in place, and as the source.  A row offset kept in 32 bits lands in another row's neighbourhood or in the lead, and
    every byte outside the three rows' pixels must still hold the fill."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h, pitch = 64, 3, (1 << 31) - 256
    words = np.ascontiguousarray(noise(RGB10A2)[:h, :w])
    (h17, d17), (h33, d33) = table(torch, 17), table(torch, 33)
    hb = HL.HugeBuffer(torch, (h - 1) * pitch + 4 * w, 1)
    try:
        assert HL.LEAD + (h - 1) * pitch > 1 << 32
        src = torch.from_numpy(words.view(np.int32)).cuda()
        view = hb.rows(0, h, 4 * w, pitch)
        api.lut3d_pass(src, 4 * w, RGB10A2, w, h, d17, 17, hb.ptr, pitch, RGB10A2)
        torch.cuda.synchronize()
        first = LM.apply(words, h17, 17, RGB10A2, RGB10A2)
        assert np.array_equal(hb.read(view).view(np.uint32), first), "as the destination"
        api.lut3d_pass(hb.ptr, pitch, RGB10A2, w, h, d33, 33, hb.ptr, pitch, BGRA8)
        torch.cuda.synchronize()
        second = LM.apply(first, h33, 33, RGB10A2, BGRA8)
        assert np.array_equal(hb.read(view).view(np.uint32), second), "in place"
        out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        api.lut3d_pass(hb.ptr, pitch, BGRA8, w, h, d17, 17, out, 4 * w, RGB10A2)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), LM.apply(second, h17, 17, BGRA8, RGB10A2)), "as the source"
        hb.assert_rest_intact([view], "3 rows at a pitch of 2^31 - 256", pitch)
    finally:
        hb.free()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h, n = 16, 8, 5
    host = random_table(n, 77)
    before = pattern(1 << 15)
    buf = torch.from_numpy(before).cuda()
    base = buf.data_ptr()
    assert base % 256 == 0
    # the source at +4096, the destination at +8192, the table (5^3 * 8 = 1000 bytes) at +16384, all inside the patterned buffer
    s0, d0, t0 = base + 4096, base + 8192, base + 16384
    buf[16384:16384 + host.nbytes] = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    start = buf.cpu().numpy()

    def call(s=s0, sp=w * 4, sf=BGRA8, w=w, h=h, t=t0, n=n, d=d0, dp=w * 4, df=RGB10A2):
        return L.mpcvr_lut3d_pass(C.c_void_p(s), sp, sf, w, h, C.c_void_p(t), n, C.c_void_p(d), dp, df, None)

    E = api.E_INVALIDARG
    for kw, hr in ((dict(s=None), api.E_POINTER), (dict(t=None), api.E_POINTER), (dict(d=None), api.E_POINTER),
                   (dict(sf=2), E), (dict(df=2), E), (dict(sf=-1), E), (dict(w=0), E), (dict(h=0), E), (dict(w=32769), E), (dict(h=32769), E),
                   (dict(n=1), E), (dict(n=0), E), (dict(n=66), E), (dict(sp=60), E), (dict(dp=60), E), (dict(sp=66), E), (dict(dp=66), E),
                   (dict(s=s0 + 2), E), (dict(d=d0 + 1), E), (dict(t=t0 + 4), E),
                   (dict(d=s0 + 4), E), (dict(d=s0 + 64), E), (dict(d=s0, dp=128, sp=64), E), (dict(d=s0 - 7 * 64 - 60), E), (dict(d=s0 + 7 * 64 + 60), E),      # over the source, not in place
                   (dict(t=d0), E), (dict(t=d0 + 7 * 64 + 56), E), (dict(d=t0 + 992), E), (dict(d=t0 - 7 * 64 - 60), E)):                                   # the table over the destination
        assert call(**kw) == hr, kw
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), start), "a refused call wrote"
    # ... and the arguments they were derived from are accepted; so is a table that overlaps the SOURCE (both are only read), and in place
    assert call() == 0
    assert call(d=d0 + 1024, t=s0) == 0
    assert call(d=s0 + 2048, s=s0 + 2048) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    words = start[4096:4096 + 4 * w * h].view(np.uint32).reshape(h, w)
    want = LM.place(start.copy(), 8192, LM.apply(words, host, n, BGRA8, RGB10A2), 4 * w)
    as_table = start[4096:4096 + 1000].view(np.uint16).reshape(-1, 4)
    LM.place(want, 8192 + 1024, LM.apply(words, as_table, n, BGRA8, RGB10A2), 4 * w)
    LM.place(want, 4096 + 2048, LM.apply(start[6144:6144 + 4 * w * h].view(np.uint32).reshape(h, w), host, n, BGRA8, RGB10A2), 4 * w)
    assert np.array_equal(got, want)
