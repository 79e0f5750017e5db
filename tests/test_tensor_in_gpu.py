"""k_sample_from_tensor (extension: a model's float tensor as a planar RGB sample, include/mpcvr.h: mpcvr_sample_pass) on the GPU: every
instantiation word for word against the numpy model (tests/tensor_in_model.py) at the shapes where the kernel takes another path, every fp16
and bf16 pattern, the named fp32 rows and the elements that tell a fused multiply-add from two roundings, every alignment of tensor and
sample inside a patterned buffer whose every other byte must survive, planes and rows more than 4 GiB apart, the refusals,
mpcvr_copy_sample_tensor against mpcvr_sample_pass + mpcvr_copy_sample, and the round trip with mpcvr_tensor_pass.  Everything is bits: no
tolerance anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import tensor_in_cases as K
from tests import tensor_in_model as M
from tests import tensor_model as TM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE_NAME = {M.F32: "f32", M.F16: "f16", M.BF16: "bf16"}
FORMAT_NAME = {M.GBRP8: "gbrp8", M.GBRP10: "gbrp10", M.GBRP16: "gbrp16"}
# (the kernel has 3 x 2 x 2 instantiations; GBRP10 is the 16-bit one with another maxcode, and runs as a case of its own)
CASES = [(d, l, f) for d in (M.F32, M.F16, M.BF16) for l in (M.PLANAR, M.INTERLEAVED) for f in K.FORMATS]
CASE_IDS = ["%s-%s-%s" % (DTYPE_NAME[d], "hwc" if l else "chw", FORMAT_NAME[f]) for d, l, f in CASES]
INSTANTIATIONS = [c for c in CASES if c[2] != M.GBRP10]
INSTANTIATION_IDS = [i for c, i in zip(CASES, CASE_IDS) if c[2] != M.GBRP10]


def tile():
    """(columns of a wavefront, columns of a workgroup, rows of a workgroup), the constants vp_tensor_in.h exports"""
    text = open(os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_tensor_in.h")).read()
    v = {k: int(n) for k, n in re.findall(r"constexpr int (kSample\w+) = (\d+);", text)}
    assert re.search(r"kSampleGroupCols = kSampleWaveCols;", text) and re.search(r"kSampleGroupRows = kSampleWaves \* kSampleWaveRows;", text)
    return v["kSampleWaveCols"], v["kSampleWaveCols"], v["kSampleWaves"] * v["kSampleWaveRows"]


WAVE_COLS, GROUP_COLS, GROUP_ROWS = tile()
WIDTHS = sorted({1, 2, 3, 4, 5, 7, 8, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, GROUP_COLS + 1})
HEIGHTS = (1, 2, GROUP_ROWS + 1)


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


_noise = {}


def noise(dtype):
    """(3, max height, max width) element bits: raw random bit patterns (NaNs, infinities, subnormals, every exponent) with every second
    element a value whose code under the ImageNet factors falls inside or just outside the format.  Smaller frames are its top-left corner."""
    if dtype not in _noise:
        h, w = max(HEIGHTS), max(WIDTHS) + 2
        rng = np.random.default_rng(900 + dtype)
        if dtype == M.F32:
            raw = rng.integers(0, 1 << 32, size=3 * h * w, dtype=np.uint64).astype(np.uint32)
            val = (rng.random(3 * h * w, dtype=np.float32) * np.float32(5.2) - np.float32(2.4)).view(np.uint32)
        else:
            raw = rng.integers(0, 1 << 16, size=3 * h * w, dtype=np.uint64).astype(np.uint16)
            v32 = (rng.random(3 * h * w, dtype=np.float32) * np.float32(5.2) - np.float32(2.4))
            val = v32.astype(np.float16).view(np.uint16) if dtype == M.F16 else (v32.view(np.uint32) >> 16).astype(np.uint16)
        raw[1::2] = val[1::2]
        _noise[dtype] = raw.reshape(3, h, w)
    return _noise[dtype]


def frame(dtype, layout, h, w):
    t = np.ascontiguousarray(noise(dtype)[:, :h, :w])
    return t if layout == M.PLANAR else np.ascontiguousarray(t.transpose(1, 2, 0))


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 17) & 255).astype(np.uint8)


def run_pass(torch, tbits, dtype, layout, order, cformat, scale=None, bias=None, src_off=0, row_pitch=None, plane_pad=0, dst_off=0, pitch=None):
    """One mpcvr_sample_pass of the tensor `tbits` ((3, h, w) / (h, w, 3) element bits) from src_off bytes behind a 256-byte boundary into a
    sample dst_off bytes behind one, inside a patterned buffer with a guard of one pitch + 4 KiB in front and behind.  Asserts the WHOLE
    buffer: the sample's pixels equal the model's codes, every other byte (pitch padding, guards) holds the pattern; the tensor is unchanged."""
    from videorenderer_amd import api
    if scale is None:
        scale, bias = K.imagenet_factors(cformat)
    h, w = (tbits.shape[1], tbits.shape[2]) if layout == M.PLANAR else (tbits.shape[0], tbits.shape[1])
    es, by = M.ELEMENT_SIZE[dtype], M.BYTES[cformat]
    row_pitch = row_pitch or es * w * (1 if layout == M.PLANAR else 3)
    plane_pitch = row_pitch * h + plane_pad if layout == M.PLANAR else 0
    host = np.full(256 + src_off + (3 * plane_pitch if layout == M.PLANAR else h * row_pitch), 0xa5, dtype=np.uint8)
    TM.place(host, 256 + src_off, tbits, layout, row_pitch, plane_pitch)
    src = torch.from_numpy(host).cuda()
    pitch = pitch or w * by
    guard = (pitch + 4096 + 255) // 256 * 256
    total = guard + dst_off + 3 * pitch * h + guard
    before = pattern(total)
    buf = torch.from_numpy(before).cuda()
    assert src.data_ptr() % 256 == 0 and buf.data_ptr() % 256 == 0
    d = api.tensor_desc(dtype, layout, row_pitch, plane_pitch, scale, bias, order)
    api.sample_pass(src.data_ptr() + 256 + src_off, d, w, h, cformat, buf.data_ptr() + guard + dst_off, pitch, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = M.place(before.copy(), guard + dst_off, M.sample(tbits, dtype, layout, order, cformat, scale, bias), pitch)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        off = int(bad[0]) - guard - dst_off
        raise AssertionError("%dx%d %s layout %d order %d -> %s, tensor +%d row pitch %d plane pitch %d, sample +%d pitch %d: %d bytes differ, the first "
                             "%d bytes from the sample's first (got %#x, want %#x, pattern %#x)"
                             % (w, h, DTYPE_NAME[dtype], layout, order, FORMAT_NAME[cformat], src_off, row_pitch, plane_pitch, dst_off, pitch, bad.size, off,
                                got[bad[0]], want[bad[0]], before[bad[0]]))
    assert src.cpu().numpy().tobytes() == host.tobytes()


@pytest.mark.parametrize("dtype,layout,cformat", CASES, ids=CASE_IDS)
def test_every_instantiation_equals_the_model_word_for_word(mpcvr, torch_cuda, dtype, layout, cformat):
    """every width and height at which a lane, a wavefront or a workgroup begins or ends, both channel orders, tight tensor and sample"""
    for h in HEIGHTS:
        for w in WIDTHS:
            for order in (M.RGB, M.BGR):
                run_pass(torch_cuda, frame(dtype, layout, h, w), dtype, layout, order, cformat)


@pytest.mark.parametrize("cformat", K.FORMATS, ids=[FORMAT_NAME[f] for f in K.FORMATS])
@pytest.mark.parametrize("layout", [M.PLANAR, M.INTERLEAVED], ids=["chw", "hwc"])
@pytest.mark.parametrize("dtype", [M.F16, M.BF16], ids=["f16", "bf16"])
def test_every_16_bit_pattern_through_the_kernel(mpcvr, torch_cuda, dtype, layout, cformat):
    """all 65,536 patterns as a 256 x 256 frame, in every channel (each channel starts elsewhere), under the ImageNet factors and the identity"""
    every = np.arange(1 << 16, dtype=np.uint32)
    t = np.stack([np.roll(every, 21845 * k) for k in range(3)]).astype(np.uint16).reshape(3, 256, 256)
    if layout == M.INTERLEAVED:
        t = np.ascontiguousarray(t.transpose(1, 2, 0))
    run_pass(torch_cuda, t, dtype, layout, M.RGB, cformat)
    run_pass(torch_cuda, t, dtype, layout, M.BGR, cformat, *K.identity_factors(cformat))


@pytest.mark.parametrize("cformat", K.FORMATS, ids=[FORMAT_NAME[f] for f in K.FORMATS])
def test_the_named_fp32_rows_through_the_kernel(mpcvr, torch_cuda, cformat):
    """the table of tests/tensor_in_cases.py: zeros, subnormals, ties, maxcode -+ 0.5, NaNs, infinities, the largest finite value under the
    factors (1, 0); the rows with factors of their own (inf * 0, subnormal products, overflow) one launch each"""
    row = np.array([b for _, b in K.named_rows(cformat)], dtype=np.uint32)
    for layout in (M.PLANAR, M.INTERLEAVED):
        t = np.stack([row, np.roll(row, 1), np.roll(row, 2)]).reshape(3, 1, -1)
        t = t if layout == M.PLANAR else np.ascontiguousarray(t.transpose(1, 2, 0))
        run_pass(torch_cuda, t, M.F32, layout, M.RGB, cformat, (1.0,) * 3, (0.0,) * 3)
        for name, b, scale, bias in K.FACTOR_ROWS:
            t = np.full((3, 1, 5) if layout == M.PLANAR else (1, 5, 3), b, dtype=np.uint32)
            run_pass(torch_cuda, t, M.F32, layout, M.RGB, cformat, (scale,) * 3, (bias,) * 3)


def test_the_elements_a_fused_multiply_add_would_change(mpcvr, torch_cuda):
    """the elements tests/test_tensor_in.py found (two roundings and one give different codes) through the kernel, each in its channel"""
    rows = K.fma_sensitive()
    assert len(rows) >= 16
    per = [[b for b, ch, _, _ in rows if ch == k] for k in range(3)]
    n = max(len(p) for p in per)
    assert min(len(p) for p in per) > 0
    t = np.stack([np.resize(np.array(p, dtype=np.uint32), n) for p in per]).reshape(3, 1, n)
    scale, bias = K.imagenet_factors(M.GBRP16)
    # (what the model says about them is what the CPU test recorded: the two-rounding code, one off the fused one)
    want = M.sample(t, M.F32, M.PLANAR, M.RGB, M.GBRP16, scale, bias)
    for k, p in enumerate(per):
        two = {b: c for b, ch, c, _ in rows if ch == k}
        assert [int(x) for x in want[(1, 2, 0).index(k), 0, :len(p)]] == [two[b] for b in p]
    for layout in (M.PLANAR, M.INTERLEAVED):
        run_pass(torch_cuda, t if layout == M.PLANAR else np.ascontiguousarray(t.transpose(1, 2, 0)), M.F32, layout, M.RGB, M.GBRP16, scale, bias)


@pytest.mark.parametrize("dtype,layout,cformat", INSTANTIATIONS, ids=INSTANTIATION_IDS)
def test_alignments_and_pitches_leave_every_other_byte_alone(mpcvr, torch_cuda, dtype, layout, cformat):
    """Tensor at +0 / +one element / +4 / +8 off a 16-byte boundary with rows tight, padded to 16 + 64 and padded by ONE element, planes
    padded by one element (the vector loads step aside); sample at +0 / +one component / +4 / +8 with a tight pitch, one padded to 16 + 16 and
    one padded by one component pair (the vector stores step aside): the same codes, and the pattern around them survives.  13 columns:
    three full lanes and a tail; wave columns + 3: a second wavefront piece of three columns."""
    es, by = M.ELEMENT_SIZE[dtype], M.BYTES[cformat]
    per = es * (1 if layout == M.PLANAR else 3)
    n = 0
    for w, h in ((13, 3), (WAVE_COLS + 3, 2)):
        t = frame(dtype, layout, h, w)
        tight = per * w
        for src_off in sorted({0, es, 4, 8}):
            for row_pitch, plane_pad in ((tight, 0), ((tight + 15) // 16 * 16 + 64, 0), (tight + es, es)):
                for dst_off in sorted({0, by, 4, 8}):
                    for pitch in (w * by + (w * by & (by - 1)), (w * by + 15) // 16 * 16 + 16, w * by + 2):
                        run_pass(torch_cuda, t, dtype, layout, (n >> 1) & 1, cformat, src_off=src_off, row_pitch=row_pitch,
                                 plane_pad=plane_pad if layout == M.PLANAR else 0, dst_off=dst_off, pitch=pitch)
                        n += 1


# ---- planes and rows more than 4 GiB apart ------------------------------------------------------------------------------------------------
FAR = (1 << 32) + 4096
FAR_GUARD = 1 << 16                        # patterned bytes in front of and behind every written row
FAR_PITCH = 1431657130                     # a sample pitch (it is an int32) of which three rows are a plane: planes 2^32 + 4094 bytes apart


@pytest.fixture(scope="module")
def far_buffer(torch_cuda):
    """one allocation for the module: a sample of three rows per plane with its planes more than 4 GiB apart, and a guard (10.7 GiB: a
    sample's pitch is an int32, so a plane that far from the next takes at least three rows of a third of 4 GiB).  Only the neighbourhoods
    of rows are ever filled or read."""
    torch = torch_cuda
    torch.cuda.empty_cache()
    buf = torch.empty(8 * FAR_PITCH + 3 * FAR_GUARD, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


def far_tensor(torch, buf, tbits, layout, row_pitch, plane_pitch):
    """the tensor's rows into buf + FAR_GUARD at the given pitches"""
    rows = [(k * plane_pitch + y * row_pitch, tbits[k, y]) for k in range(3) for y in range(tbits.shape[1])] if layout == M.PLANAR else \
           [(y * row_pitch, tbits[y].reshape(-1)) for y in range(tbits.shape[0])]
    for off, row in rows:
        b = torch.from_numpy(np.ascontiguousarray(row).view(np.uint8)).cuda()
        buf[FAR_GUARD + off:FAR_GUARD + off + b.numel()] = b


@pytest.mark.parametrize("dtype,cformat", [(M.F16, M.GBRP8), (M.F32, M.GBRP16), (M.BF16, M.GBRP10)], ids=["f16-gbrp8", "f32-gbrp16", "bf16-gbrp10"])
def test_tensor_planes_more_than_4_gib_apart(mpcvr, torch_cuda, far_buffer, dtype, cformat):
    """64 x (group rows + 1), C,H,W, the three planes 2^32 + 4096 bytes apart: a plane offset kept in 32 bits reads the first plane's neighbourhood"""
    from videorenderer_amd import api
    torch = torch_cuda
    t = frame(dtype, M.PLANAR, GROUP_ROWS + 1, 64)
    rp = 64 * M.ELEMENT_SIZE[dtype] + 64
    far_tensor(torch, far_buffer, t, M.PLANAR, rp, FAR)
    scale, bias = K.imagenet_factors(cformat)
    out = torch.zeros(3 * (GROUP_ROWS + 1) * 64 * M.BYTES[cformat], dtype=torch.uint8, device="cuda")
    api.sample_pass(far_buffer.data_ptr() + FAR_GUARD, api.tensor_desc(dtype, M.PLANAR, rp, FAR, scale, bias, M.BGR), 64, GROUP_ROWS + 1, cformat, out, 64 * M.BYTES[cformat], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = M.sample(t, dtype, M.PLANAR, M.BGR, cformat, scale, bias)
    assert out.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype,layout,cformat", [(M.F16, M.INTERLEAVED, M.GBRP16), (M.F32, M.INTERLEAVED, M.GBRP8), (M.BF16, M.PLANAR, M.GBRP16)],
                         ids=["f16-hwc-gbrp16", "f32-hwc-gbrp8", "bf16-chw-gbrp16"])
def test_tensor_rows_more_than_4_gib_apart(mpcvr, torch_cuda, far_buffer, dtype, layout, cformat):
    """Rows 2^32 + 4096 bytes apart.  Three rows of 64 columns (the second row of a wavefront and the first of the next; the C,H,W case
    keeps its planes a row apart inside the first row's neighbourhood): a row offset kept in 32 bits shows at the second row already."""
    from videorenderer_amd import api
    torch = torch_cuda
    t = frame(dtype, layout, 3, 64)
    pp = 1024 if layout == M.PLANAR else 0
    far_tensor(torch, far_buffer, t, layout, FAR, pp)
    scale, bias = K.imagenet_factors(cformat)
    out = torch.zeros(3 * 3 * 64 * M.BYTES[cformat], dtype=torch.uint8, device="cuda")
    api.sample_pass(far_buffer.data_ptr() + FAR_GUARD, api.tensor_desc(dtype, layout, FAR, pp, scale, bias, M.RGB), 64, 3, cformat, out, 64 * M.BYTES[cformat], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = M.sample(t, dtype, layout, M.RGB, cformat, scale, bias)
    assert out.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype,layout,cformat", [(M.F16, M.PLANAR, M.GBRP16), (M.F32, M.INTERLEAVED, M.GBRP8)], ids=["f16-chw-gbrp16", "f32-hwc-gbrp8"])
def test_sample_planes_more_than_4_gib_apart(mpcvr, torch_cuda, far_buffer, dtype, layout, cformat):
    """A 64 x 3 sample at a pitch of a third of 2^32 + 4094: its planes lie more than 4 GiB apart (a plane offset kept in 32 bits lands
    4094 bytes behind plane G) and its rows 1.33 GiB.  Every written row is read back with half a guard in front and behind, which must hold the pattern."""
    from videorenderer_amd import api
    torch = torch_cuda
    buf = far_buffer
    t = frame(dtype, layout, 3, 64)
    scale, bias = K.imagenet_factors(cformat)
    codes = M.sample(t, dtype, layout, M.RGB, cformat, scale, bias)
    half = FAR_GUARD // 2
    rows = [((p * 3 + y) * FAR_PITCH, np.ascontiguousarray(codes[p, y]).view(np.uint8)) for p in range(3) for y in range(3)]
    for off, _ in rows:
        buf[FAR_GUARD + off - half:FAR_GUARD + off + half] = torch.from_numpy(pattern(FAR_GUARD)).cuda()
    src = torch.from_numpy(t.view(np.uint8).reshape(-1)).cuda()
    es = M.ELEMENT_SIZE[dtype]
    rp = 64 * es * (3 if layout == M.INTERLEAVED else 1)
    api.sample_pass(src, api.tensor_desc(dtype, layout, rp, rp * 3, scale, bias, M.RGB), 64, 3, cformat, buf.data_ptr() + FAR_GUARD, FAR_PITCH, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for off, row in rows:
        got = buf[FAR_GUARD + off - half:FAR_GUARD + off + half].cpu().numpy()
        want = pattern(FAR_GUARD)
        want[half:half + row.size] = row
        assert np.array_equal(got, want), ("row at byte %d of the sample" % off, np.nonzero(got != want)[0][:8])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h = 16, 8
    src = torch.zeros(3 * h * w * 2 + 64, dtype=torch.uint8, device="cuda")         # fp16 zeros
    before = pattern(1 << 14)
    buf = torch.from_numpy(before).cuda()
    t0, s0 = src.data_ptr(), buf.data_ptr() + 4096

    def call(tensor=t0, sample=s0, w=w, h=h, cformat=M.GBRP8, pitch=None, desc=True, dtype=M.F16, layout=M.PLANAR, order=M.RGB, reserved=0,
             row_pitch=None, plane_pitch=None, scale=(255.0,) * 3, bias=(3.0,) * 3):
        es = M.ELEMENT_SIZE.get(dtype, 2)
        rp = row_pitch if row_pitch is not None else es * 16 * (1 if layout == M.PLANAR else 3)
        d = api.tensor_desc(dtype, layout, rp, plane_pitch if plane_pitch is not None else rp * 8, scale, bias, order)
        d.reserved = reserved
        return L.mpcvr_sample_pass(C.c_void_p(tensor), C.byref(d) if desc else None, w, h, cformat, C.c_void_p(sample),
                                   pitch if pitch is not None else 16 * M.BYTES.get(cformat, 1), None)

    E = api.E_INVALIDARG
    for kw, hr in ((dict(tensor=None), api.E_POINTER), (dict(sample=None), api.E_POINTER), (dict(desc=False), api.E_POINTER),
                   (dict(cformat=0), E), (dict(cformat=25), E), (dict(cformat=29), E), (dict(w=0), E), (dict(h=0), E), (dict(w=32769), E), (dict(h=32769), E),
                   (dict(dtype=3), E), (dict(layout=2), E), (dict(order=2), E), (dict(reserved=7), E),
                   (dict(scale=(1.0, float("inf"), 1.0)), E), (dict(scale=(float("nan"), 1.0, 1.0)), E), (dict(scale=(1.0, 1.0, 2.0 ** 101)), E),
                   (dict(scale=(2.0 ** -101, 1.0, 1.0)), E), (dict(bias=(0.0, float("nan"), 0.0)), E), (dict(bias=(0.0, 0.0, -(2.0 ** 101))), E),
                   (dict(row_pitch=30), E), (dict(row_pitch=0), E), (dict(row_pitch=-32), E), (dict(row_pitch=33), E), (dict(row_pitch=(1 << 47) + 2), E),
                   (dict(layout=M.INTERLEAVED, row_pitch=94), E), (dict(plane_pitch=0), E), (dict(plane_pitch=-256), E), (dict(plane_pitch=257), E),
                   (dict(plane_pitch=(1 << 47) + 2), E), (dict(tensor=t0 + 1), E), (dict(dtype=M.F32, tensor=t0 + 2), E),
                   (dict(pitch=15), E), (dict(cformat=M.GBRP16, pitch=30), E), (dict(cformat=M.GBRP10, pitch=33), E), (dict(cformat=M.GBRP16, sample=s0 + 1), E),
                   (dict(tensor=s0), E), (dict(tensor=s0 + 3 * 128 - 2), E), (dict(tensor=s0 - 768 + 2), E), (dict(layout=M.INTERLEAVED, tensor=s0 + 256), E)):      # over the sample
        assert call(**kw) == hr, kw
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before) and not bool(src.any())
    assert call() == 0          # ... and the arguments they were derived from are accepted
    torch.cuda.synchronize()
    want = M.place(before.copy(), 4096, np.full((3, h, w), 3, dtype=np.uint8), 16)
    assert np.array_equal(buf.cpu().numpy(), want)


# ---- mpcvr_copy_sample_tensor -------------------------------------------------------------------------------------------------------------
def _context(api, cformat, w, h, scale2, flags, own_stream=False):
    vp = api.VideoProcessor(api.default_settings(iUpscaling=2, flags=flags), use_torch_stream=not own_stream)
    vp.InitMediaType(cformat, w, h)
    vp.SetWindowRect((0, 0, w * scale2, h * scale2))
    vp.SetVideoRect((0, 0, w * scale2, h * scale2))
    return vp


def _picture(torch, rng, dtype, layout, w, h):
    """a float picture in [-0.1, 1.1] as a torch tensor of the dtype and layout"""
    a = (rng.random((3, h, w), dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
    t = torch.from_numpy(a if layout == M.PLANAR else np.ascontiguousarray(a.transpose(1, 2, 0))).cuda()
    return t.to({M.F32: torch.float32, M.F16: torch.float16, M.BF16: torch.bfloat16}[dtype])


def _composition(api, torch, t, cformat, w, h, scale2, flags, scale, bias, order="rgb"):
    """mpcvr_sample_pass into a caller's buffer, mpcvr_copy_sample(MPCVR_MEM_DEVICE), mpcvr_process"""
    vp = _context(api, cformat, w, h, scale2, flags)
    nbytes, pitch = vp.GetFrameBytes()
    smp = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d, tw, th = api._frame_tensor_desc(t, scale, bias, order)
    assert (tw, th) == (w, h)
    api.sample_pass(t, d, w, h, cformat, smp, pitch, torch.cuda.current_stream().cuda_stream)
    dst = torch.zeros((h * scale2, w * scale2, 4), dtype=torch.uint8, device="cuda")
    vp.CopySample(smp, pitch)
    vp.Process(dst, w * scale2 * 4)
    vp.Synchronize()
    out = dst.cpu().numpy()
    vp.close()
    return out


@pytest.mark.parametrize("w,h", [(16, 8), (64, 32)], ids=["16x8", "64x32"])
@pytest.mark.parametrize("tier", ["default", "no_fused"])
@pytest.mark.parametrize("scale2", [1, 2], ids=["same_size", "2x"])
def test_copy_sample_tensor_then_process_equals_the_composition(mpcvr, torch_cuda, scale2, tier, w, h):
    from videorenderer_amd import api
    torch = torch_cuda
    flags = api.FLAG_NO_FUSED if tier == "no_fused" else 0
    rng = np.random.default_rng(w * 10 + scale2)
    for cformat, dtype, layout, order in ((M.GBRP16, M.F16, M.PLANAR, "rgb"), (M.GBRP8, M.F32, M.INTERLEAVED, "bgr"), (M.GBRP10, M.BF16, M.PLANAR, "rgb")):
        scale, bias = K.identity_factors(cformat)
        t = _picture(torch, rng, dtype, layout, w, h)
        want = _composition(api, torch, t, cformat, w, h, scale2, flags, scale, bias, order)
        vp = _context(api, cformat, w, h, scale2, flags)
        dst = torch.zeros((h * scale2, w * scale2, 4), dtype=torch.uint8, device="cuda")
        vp.CopySampleTensor(t, scale, bias, order)
        vp.Process(dst, w * scale2 * 4)
        vp.Synchronize()
        got = dst.cpu().numpy()
        vp.close()
        assert want.any() and np.array_equal(got, want), (FORMAT_NAME[cformat], DTYPE_NAME[dtype], int((got != want).sum()))


def test_four_tensor_samples_in_a_row_on_a_context_that_owns_its_stream(mpcvr, torch_cuda):
    """Slot ring (three slots: the fourth sample takes the first one's) and frame lanes.  The context owns its stream, so nothing of torch's
    can be queued on it: each tensor is overwritten once the host has waited for the pass (Synchronize) and BEFORE its Process is queued —
    the frame must come from the slot, not from the tensor — and the four Process calls stay in flight on the lanes together."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h, cformat = 64, 32, M.GBRP16
    scale, bias = K.identity_factors(cformat)
    rng = np.random.default_rng(44)
    ts = [_picture(torch, rng, M.F16, M.PLANAR, w, h) for _ in range(4)]
    want = [_composition(api, torch, t, cformat, w, h, 2, 0, scale, bias) for t in ts]
    assert not np.array_equal(want[0], want[1])
    torch.cuda.synchronize()
    vp = _context(api, cformat, w, h, 2, 0, own_stream=True)
    dsts = [torch.zeros((2 * h, 2 * w, 4), dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for t, dst in zip(ts, dsts):
        vp.CopySampleTensor(t, scale, bias)
        vp.Synchronize()
        t.fill_(0.5)
        torch.cuda.synchronize()
        vp.Process(dst, 2 * w * 4)
    vp.Synchronize()
    for i in range(4):
        assert np.array_equal(dsts[i].cpu().numpy(), want[i]), i
    vp.close()


def test_copy_sample_tensor_refusals_keep_the_previous_sample(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    w, h = 16, 8
    t = _picture(torch, np.random.default_rng(3), M.F16, M.PLANAR, w, h)
    L = api.load_library()
    vp = api.VideoProcessor(api.default_settings())
    d, _, _ = api._frame_tensor_desc(t, (255.0,) * 3, (0.0,) * 3, "rgb")
    assert L.mpcvr_copy_sample_tensor(vp._ctx, C.c_void_p(t.data_ptr()), C.byref(d)) == api.E_NOT_VALID_STATE
    vp.InitMediaType(1, w, h)                        # not a planar RGB input
    assert L.mpcvr_copy_sample_tensor(vp._ctx, C.c_void_p(t.data_ptr()), C.byref(d)) == api.E_INVALIDARG
    vp.close()
    vp = _context(api, M.GBRP8, w, h, 1, 0)
    dst = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    vp.CopySampleTensor(t)
    vp.Process(dst, w * 4)
    vp.Synchronize()
    first = dst.cpu().numpy().copy()
    assert L.mpcvr_copy_sample_tensor(vp._ctx, None, C.byref(d)) == api.E_POINTER
    assert L.mpcvr_copy_sample_tensor(vp._ctx, C.c_void_p(t.data_ptr()), None) == api.E_POINTER
    bad = api.tensor_desc(M.F16, M.PLANAR, d.row_pitch, d.plane_pitch, (float("inf"),) * 3, (0.0,) * 3)
    assert L.mpcvr_copy_sample_tensor(vp._ctx, C.c_void_p(t.data_ptr()), C.byref(bad)) == api.E_INVALIDARG
    assert L.mpcvr_copy_sample_tensor(vp._ctx, C.c_void_p(t.data_ptr() + 1), C.byref(d)) == api.E_INVALIDARG
    dst.zero_()
    vp.Process(dst, w * 4)                           # the previous sample is still current
    vp.Synchronize()
    assert first.any() and np.array_equal(dst.cpu().numpy(), first)
    vp.close()


# ---- round trip at 8 bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [M.F32, M.F16], ids=["f32", "f16"])
def test_round_trip_at_8_bits(mpcvr, torch_cuda, dtype):
    """A BGRA8 frame through mpcvr_tensor_pass (scale 1 / 255) and back through mpcvr_sample_pass (scale 255, GBRP8) is the frame's own
    codes: code / 255 in fp32 or fp16 is within 2^-12 of the quotient, times 255 within 0.07 of the code.  First on the CPU through the two
    models over every code, then through the two kernels.  bf16 is not claimed: its 8 significant bits leave up to half a code."""
    from videorenderer_amd import api
    torch = torch_cuda
    every = np.arange(256, dtype=np.uint32)
    back = M.code(TM.element_bits(every, 1 / 255, 0.0, dtype), dtype, M.GBRP8, 255.0, 0.0)
    assert np.array_equal(back, every)
    w, h = WAVE_COLS + 5, GROUP_ROWS + 1
    rng = np.random.default_rng(8)
    words = rng.integers(0, 1 << 32, size=(h, w), dtype=np.uint64).astype(np.uint32)
    src = torch.from_numpy(words.view(np.int32)).cuda()
    es = M.ELEMENT_SIZE[dtype]
    for layout in (M.PLANAR, M.INTERLEAVED):
        rp = es * w * (3 if layout == M.INTERLEAVED else 1)
        mid = torch.zeros(3 * h * w * es, dtype=torch.uint8, device="cuda")
        out = torch.zeros(3 * h * w, dtype=torch.uint8, device="cuda")
        api.tensor_pass(src, 4 * w, TM.BGRA8, w, h, api.tensor_desc(dtype, layout, rp, rp * h, (1 / 255,) * 3, (0.0,) * 3), mid, torch.cuda.current_stream().cuda_stream)
        api.sample_pass(mid, api.tensor_desc(dtype, layout, rp, rp * h, (255.0,) * 3, (0.0,) * 3), w, h, M.GBRP8, out, w, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        c = TM.codes(words, TM.BGRA8)               # R, G, B
        want = np.stack([c[1], c[2], c[0]]).astype(np.uint8)
        assert out.cpu().numpy().tobytes() == want.tobytes()
