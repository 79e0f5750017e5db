"""How a sample is READ: row pitch, plane offsets, poisoned padding (tests/sample_layouts.py lays the samples out; tests/test_sample_layouts.py
shows on the CPU that the oracle reads no padding byte and which RGB texels a pitch fills).

For every (route, format, pitch class) one context per tier is set up with InitMediaType(..., pitch=P) and draws the same picture twice, its
padding poisoned with two different byte patterns:
  (a) poison A == poison B, bit for bit, on the default tier and on the plain tier (MPCVR_FLAG_NO_FUSED, the tier of
      test_pass_per_kernel_path_vs_oracle): a difference is a padding byte that reached a pixel;
  (b) padded == tight, bit for bit, wherever GetVPInfo names the same kernel for both, and always on the plain tier — except for the interleaved
      RGB formats at pitches whose copy loops fill other texels than the tight pitch's (tests/sample_layouts.py::rgb_texels_written);
  (c) padded against oracle.process(p, padded sample, P) at the bar the route has in tests/test_parity_gpu.py: the plain tier exact, the other
      tiers `compare` (<= 1 code, >= 99 % identical), behind a PQ tail `compare_behind_tail` with its defaults;
  (d) the route: GetVPInfo of the tight sample names the kernel the case is meant for, and a pitch class keeps it exactly where the kernel's
      loads can take the layout (fast_convert of CHipVideoProcessor::FillFusedParams, restated in takes_fast_convert below) — where they
      cannot, the info must NOT name it.

Pitch classes (tests/sample_layouts.py::pitch_of; T = the tight row): wide (next multiple of 256 above T), mod16=8, mod8=4, mod4=2, odd
(1-byte samples).  GetVPInfo says "direct:convert" for the three kernels a same-size frame may take (k_convert_stream, k_convert_blocks, the
per-pixel k_convert_direct): there (d) holds the prefix, and (b) is asserted between layouts whose kernel — by the launch conditions restated in
direct_kernel below — is the same one.
"""
import numpy as np
import pytest

from tests.golden.cases import HDR10, M709, case_frame, ext, oracle_params
from tests.sample_layouts import (RGB_BPP, bottom_up, frame_bytes, pitch_of, relayout, rgb_texels_written, row_bytes, sample_bytes)
from tests.test_parity_gpu import BG, compare, compare_behind_tail, has_tail, make_vp, path_ok
from videorenderer_amd import synth

pytestmark = pytest.mark.gpu

SDR = ext(matrix=M709)
POISON_A, POISON_B = 1, 2
TIERS = ("default", "plain")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def tier_flags(tier):
    from videorenderer_amd import api
    return api.FLAG_NO_FUSED if tier == "plain" else 0


# ---- the library's own conditions, restated ------------------------------------------------------------------------------------------
def chroma_layout(cformat, h, pitch):
    """(chroma pitch, plane_off[1], plane_off[2]) as FillFusedParams derives them (one-plane formats included: the sums are formed anyway)"""
    if cformat in synth.FORMATS:
        planes, _, dw, dh = synth.FORMATS[cformat][:4]
    else:
        planes, dw, dh = (3 if synth.PACKED[cformat][0] == "gbrp" else 1), 1, 1
    cpitch = pitch // dw if planes == 3 else pitch
    return cpitch, pitch * h, pitch * h + cpitch * (h // dh)


def takes_fast_convert(cformat, h, pitch):
    """fast_convert (whole frame as the source rect): dword loads need the luma pitch, the chroma pitch and both plane offsets on multiples of 4.
    Without it the exact-2x kernels, k_fused_strip / k_fused_period on raw samples and k_convert_blocks step aside."""
    cpitch, off1, off2 = chroma_layout(cformat, h, pitch)
    return pitch % 4 == 0 and cpitch % 4 == 0 and off1 % 4 == 0 and off2 % 4 == 0


def direct_kernel(cformat, w, h, pitch):
    """the kernel behind "direct:convert" for an aligned sample and target (LaunchConvertBlocks): the streaming kernel wants 8-byte rows of P01x,
    4-byte rows of NV12, the block kernel fast_convert, and the per-pixel kernel takes the rest"""
    if not takes_fast_convert(cformat, h, pitch):
        return "k_convert_direct"
    lbs = {1: 4, 2: 8, 3: 8}.get(cformat)
    if lbs and w >= 8 and w % 4 == 0 and pitch % lbs == 0 and (pitch * h) % lbs == 0:
        return "k_convert_stream"
    return "k_convert_blocks"


FAST_KERNELS = ("fused_up2x", "fused_jinc2x", "kernel=fused_strip(", "kernel=fused_period(")      # every one of them needs fast_convert


# ---- drawing -------------------------------------------------------------------------------------------------------------------------
def padded_sample(c, pitch, poison):
    """the case's picture at |pitch| (bottom-up where pitch < 0) -> (numpy bytes, the pitch CopySample takes)"""
    frame, _ = case_frame(dict(c, bottom_up=0, pitch=None))
    buf = relayout(frame, c["cformat"], c["w"], c["h"], abs(pitch), poison)
    return bottom_up(buf, c["h"], abs(pitch)) if pitch < 0 else (buf, pitch)


def context(mpcvr, c, pitch, tier):
    vp, (ww, wh) = make_vp(mpcvr, dict(c, pitch=abs(pitch), bottom_up=0), tier_flags(tier) | c.get("lib_flags", 0))
    if pitch < 0:
        vp.InitMediaType(c["cformat"], c["w"], c["h"], pitch=pitch, extfmt=c.get("exfmt", 0))
    assert vp.GetFrameBytes() == (frame_bytes(c["cformat"], c["w"], c["h"], abs(pitch)), abs(pitch)), "GetFrameBytes reports the padded pitch and size"
    return vp, ww, wh


def draw(torch, vp, sample, pitch, ww, wh, **kw):
    dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
    vp.CopySample(sample, pitch, **kw)
    vp.Process(dst, ww * 4)
    vp.Synchronize()
    return dst.cpu().numpy()


def draw_poisons(mpcvr, torch, c, pitch, tier):
    """one context at `pitch`: the picture with poison A, with poison B -> (A, B, GetVPInfo)"""
    vp, ww, wh = context(mpcvr, c, pitch, tier)
    outs = []
    for poison in (POISON_A, POISON_B):
        buf, sp = padded_sample(c, pitch, poison)
        outs.append(draw(torch, vp, torch.from_numpy(buf).cuda(), sp, ww, wh))
    info = vp.GetVPInfo()
    vp.close()
    return outs[0], outs[1], info


_TIGHT = {}


def tight(mpcvr, torch, oracle, c, tier):
    """(pixels, GetVPInfo) of the case at the default pitch, zero padding — computed once per (case, tier), read-only; held to the oracle too"""
    key = (repr(sorted((k, repr(v)) for k, v in c.items())), tier)
    if key not in _TIGHT:
        p0 = synth.default_pitch(c["cformat"], c["w"])
        vp, ww, wh = context(mpcvr, c, p0, tier)
        buf, sp = padded_sample(c, p0, None)
        out = draw(torch, vp, torch.from_numpy(buf).cuda(), sp, ww, wh)
        info = vp.GetVPInfo()
        vp.close()
        against_oracle(oracle, c, buf, sp, out, tier, f"tight <{tier}> [{info}]")
        out.setflags(write=False)
        _TIGHT[key] = (out, info)
    return _TIGHT[key]


def against_oracle(oracle, c, sample, pitch, got, tier, what):
    """(c): the bars of tests/test_parity_gpu.py — the plain tier exact (test_pass_per_kernel_path_vs_oracle), everything else <= 1 code and
    >= 99 % identical (test_default_path_vs_oracle), behind a PQ / HLG tail through compare_behind_tail with its defaults"""
    p = oracle_params(oracle, c)
    want = oracle.process(p, sample, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    if tier == "plain":
        compare(got, want, what, exact=True)
    elif has_tail(c):
        compare_behind_tail(oracle, p, sample, pitch, got, want, what, min_same=0.99)
    else:
        compare(got, want, what, min_same=0.99)


ROUTE_LOG = []          # (route, format, class, pitch, tier, info): printed at the end of the module (pytest -s / a job script's log)


def names(info, kernel):
    """does GetVPInfo name `kernel` (a fragment, or a prefix for path_ok; k_fused_period is k_fused_strip's launch at the periodic ratios)"""
    return kernel in info or path_ok(info, kernel) or (kernel.startswith("kernel=fused_strip") and kernel.replace("fused_strip", "fused_period") in info)


def is_fast(kernel):
    return any(kernel.startswith(k) for k in FAST_KERNELS)


def kernel_key(c, info, pitch):
    """layouts with the same GetVPInfo run the same kernel iff their keys agree: "direct:convert" stands for three kernels"""
    return direct_kernel(c["cformat"], c["w"], c["h"], abs(pitch)) if info.startswith("direct:convert") else None


def check_layouts(mpcvr, torch, oracle, c, route, classes, kernel):
    """The four assertions for one case over its pitch classes (a class: a name for pitch_of, or a pitch; negative = bottom-up).  kernel: what
    GetVPInfo of the default tier must name — one of FAST_KERNELS exactly where the layout allows fast_convert (and none of them where it does
    not), anything else for every layout alike."""
    cf, w, h = c["cformat"], c["w"], c["h"]
    kind = synth.PACKED[cf][0] if cf in synth.PACKED else None
    t_pitch = synth.default_pitch(cf, w)
    refs = {tier: tight(mpcvr, torch, oracle, c, tier) for tier in TIERS}
    assert refs["plain"][1].startswith("passes:"), refs["plain"][1]
    done = 0
    for cls in ("tight",) + tuple(classes):
        pitch = cls if isinstance(cls, int) else pitch_of(cls, cf, w)
        if pitch is None:
            continue
        if cf in synth.FORMATS and synth.FORMATS[cf][:2] == (3, 2) and (pitch // synth.FORMATS[cf][2]) % 2:
            continue                    # refused by InitMediaType (test_odd_chroma_pitch_of_16_bit_planes_is_refused)
        done += cls != "tight"
        for tier in TIERS:
            ref, ref_info = refs[tier]
            if cls == "tight":
                a, b, info = ref, ref, ref_info
            else:
                a, b, info = draw_poisons(mpcvr, torch, c, pitch, tier)
            what = f"{route} cformat {cf} {w}x{h} <{cls}: pitch {pitch}> <{tier}> [{info}]"
            ROUTE_LOG.append((route, cf, str(cls), pitch, tier, info))
            # (a)
            assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} bytes depend on the padding bytes"
            # (d)
            if tier == "plain":
                assert info.startswith("passes:"), what
            elif is_fast(kernel) and not takes_fast_convert(cf, h, abs(pitch)):
                assert not any(k in info for k in FAST_KERNELS), f"{what}: a kernel with dword loads runs on rows / planes that are not dword aligned"
            else:
                assert names(info, kernel), f"{what}: expected {kernel}"
                assert is_fast(kernel) or info == ref_info, f"{what}: the tight sample runs [{ref_info}]"
            if cls == "tight":
                continue
            # (b)
            fills_the_same = kind not in synth.RGB_FAMILIES or rgb_texels_written(kind, pitch, w) == rgb_texels_written(kind, t_pitch, w)
            if fills_the_same and (tier == "plain" or (info == ref_info and kernel_key(c, info, pitch) == kernel_key(c, info, t_pitch))):
                assert np.array_equal(a, ref), f"{what}: {int((a != ref).sum())} bytes differ from the tight sample's frame"
            # (c)
            buf, sp = padded_sample(c, pitch, POISON_A)
            against_oracle(oracle, c, buf, sp, a, tier, what)
    assert done >= 2, (route, cf, classes)


ALL = ("wide", "mod16=8", "mod8=4", "mod4=2", "odd")


def case(cformat, w, h, dst, seed, exfmt=SDR, **kw):
    return dict(cformat=cformat, w=w, h=h, kind="noise", seed=seed, dst=dst, exfmt=exfmt, **kw)


# ---- exact 2x ------------------------------------------------------------------------------------------------------------------------
UP2X_SOURCES = {"p010_pq": (2, HDR10), "nv12": (1, SDR), "yv12": (14, SDR), "yuv420p10": (20, SDR), "p210": (6, SDR), "yuy2": (4, SDR),
                "y410": (12, SDR), "y8": (37, SDR)}


@pytest.mark.parametrize("taps", ["lanczos3", "catmull_rom"])
@pytest.mark.parametrize("src", sorted(UP2X_SOURCES))
def test_exact_2x(mpcvr, oracle, torch_cuda, src, taps):
    """k_fused_up2x: 136 x 24 is two 64-column strips and a partial one.  Every class with fast_convert keeps the kernel (wide, mod16=8, and mod8=4
    except for three-plane 8-bit samples, whose chroma pitch is then 2 mod 4); mod4=2 and odd send the frame to the convert kernel and the
    surface variant of the resize kernels."""
    cf, exfmt = UP2X_SOURCES[src]
    c = case(cf, 136, 24, (272, 48), 700 + cf, exfmt, iUpscaling=4 if taps == "lanczos3" else 2)
    check_layouts(mpcvr, torch_cuda, oracle, c, f"up2x/{taps}", ALL, "fused_up2x")


def test_fused_jinc_2x(mpcvr, oracle, torch_cuda):
    c = case(2, 136, 24, (272, 48), 730, SDR, iUpscaling=5)
    check_layouts(mpcvr, torch_cuda, oracle, c, "jinc2x", ALL, "fused_jinc2x")


# ---- arbitrary ratio -----------------------------------------------------------------------------------------------------------------
STRIP_SOURCES = {"p010": 2, "nv12": 1, "yv12": 14, "rgb32": 30}


@pytest.mark.parametrize("geo", ["up_1p5x", "down"])
@pytest.mark.parametrize("src", sorted(STRIP_SOURCES))
def test_fused_strip(mpcvr, oracle, torch_cuda, src, geo):
    """k_fused_strip straight from the raw sample (at 3:2 the planner would take k_fused_period, which has its own test: MPCVR_FLAG_NO_PERIOD); RGB32
    is copied into the context's texture row for row (CopyPlaneAsIs) and feeds the surface variant whatever its pitch."""
    from videorenderer_amd import api
    cf = STRIP_SOURCES[src]
    dst = (204, 36) if geo == "up_1p5x" else (100, 18)
    c = case(cf, 136, 24, dst, 740 + cf, SDR, iUpscaling=4, iDownscaling=2, lib_flags=api.FLAG_NO_PERIOD)
    check_layouts(mpcvr, torch_cuda, oracle, c, f"strip/{geo}", ALL, "kernel=fused_strip:surface(" if src == "rgb32" else "kernel=fused_strip(")


@pytest.mark.parametrize("src", ["p010_pq", "nv12"])
def test_fused_period_4_3(mpcvr, oracle, torch_cuda, src):
    cf, exfmt = UP2X_SOURCES[src]
    c = case(cf, 144, 24, (192, 32), 760 + cf, exfmt, iUpscaling=4)
    check_layouts(mpcvr, torch_cuda, oracle, c, "period/4:3", ALL, "kernel=fused_period(rows=4:3,taps=5,")


# ---- same size ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["nv12", "p010_pq"])
def test_direct_convert(mpcvr, oracle, torch_cuda, src):
    """264 x 16: one 256-column strip of k_convert_stream and a partial one.  NV12 keeps the streaming kernel down to mod8=4 and loses every block
    kernel at mod4=2 / odd; P010 hands over to k_convert_blocks at mod8=4 and to the per-pixel kernel at mod4=2 (direct_kernel)."""
    cf, exfmt = UP2X_SOURCES[src]
    c = case(cf, 264, 16, (264, 16), 770 + cf, exfmt)
    kernels = {cls: direct_kernel(cf, 264, 16, pitch_of(cls, cf, 264)) for cls in ("tight",) + ALL if pitch_of(cls, cf, 264)}
    assert kernels["tight"] == kernels["wide"] == kernels["mod16=8"] == "k_convert_stream" and kernels["mod4=2"] == "k_convert_direct"
    assert kernels["mod8=4"] == ("k_convert_stream" if cf == 1 else "k_convert_blocks")
    check_layouts(mpcvr, torch_cuda, oracle, c, "direct", ALL, "direct:convert")


# one format of every layout family of synth.FORMATS / synth.PACKED (v210 and interleaved RGB: the repack tests below)
PLAIN_FORMATS = [1, 2, 6, 14, 15, 16, 20, 22, 25, 4, 5, 8, 11, 12, 13, 26, 27, 37, 38]


@pytest.mark.parametrize("cformat", PLAIN_FORMATS)
def test_per_pixel_convert(mpcvr, oracle, torch_cuda, cformat):
    """70 x 10 at the same size: the per-pixel convert of the plain tier (and whatever the default tier takes) for every plane walk."""
    c = case(cformat, 70, 10, (70, 10), 800 + cformat)
    check_layouts(mpcvr, torch_cuda, oracle, c, "plain", ALL, "direct:convert")


@pytest.mark.parametrize("w,h", [(70, 34), (68, 36)])
@pytest.mark.parametrize("cformat", [14, 17])
def test_third_plane_offset(mpcvr, oracle, torch_cuda, cformat, w, h):
    """Three planes, 4:2:0, luma pitch 76 (4 mod 8): the chroma pitch is 38 (2 mod 4); 17 chroma rows put the third plane at 2 mod 4, 18 chroma
    rows on a multiple of 4.  Same size and 2x."""
    pitch = pitch_of("mod8=4", cformat, w)
    cpitch, off1, off2 = chroma_layout(cformat, h, pitch)
    assert (pitch, cpitch % 4, off1 % 4, off2 % 4) == (76, 2, 0, 2 if h == 34 else 0)
    for dst, kernel in (((w, h), "direct:convert"), ((2 * w, 2 * h), "fused_up2x")):
        c = case(cformat, w, h, dst, 820 + cformat + h, iUpscaling=2)
        check_layouts(mpcvr, torch_cuda, oracle, c, "plane_off[2]", ("mod8=4", "wide"), kernel)


# ---- the repacks ------------------------------------------------------------------------------------------------------------------------
def test_v210_repack(mpcvr, oracle, torch_cuda):
    """CopyFrameV210 -> Y210 texture: the default pitch (128-aligned), the next multiple of 128, a merely 4-aligned pitch, a wide one."""
    w = 70
    t = row_bytes(10, w)
    default = synth.default_pitch(10, w)
    assert default % 128 == 0 and (t + 4) % 8 == 4
    for dst in ((w, 12), (2 * w, 24)):
        c = case(10, w, 12, dst, 840, iUpscaling=2)
        check_layouts(mpcvr, torch_cuda, oracle, c, "v210", (default + 128, t + 4, t + 8, 512, default + 256 + 4), "")


RGB_SOURCES = {"rgb24": 29, "rgb32": 30, "r210": 32, "rgb48": 33, "bgr48": 34, "bgra64": 35, "b64a": 36}


def rgb_pitches(kind, cf, w):
    """pitches whose |pitch| // bpp is the width, the width + 1, + 2, + 3 (every remainder of the copy loops' groups of four) and a wide one"""
    bpp, b = RGB_BPP[kind], sample_bytes(cf)
    ps = []
    for lp in range(w, w + 4):
        p = lp * bpp
        while p % b:
            p += 1
        assert p // bpp == lp, (kind, w, lp, p)
        ps.append(p)
    assert {(p // bpp) % 4 for p in ps} == {0, 1, 2, 3}
    return ps + [pitch_of("wide", cf, w)]


@pytest.mark.parametrize("w", [45, 46, 47])
@pytest.mark.parametrize("src", sorted(RGB_SOURCES))
def test_rgb_repack(mpcvr, oracle, torch_cuda, src, w):
    """k_repack_rgb restates loops that run over |pitch| / bytes-per-pixel: widths of 4k + 1, + 2, + 3 at pitches that put that quotient on every
    remainder.  RGB48 46 wide at 288 bytes and above is the row whose last two texels the reference fills (at the tight pitch they are black);
    RGB24 46 / 47 wide at 141 .. 143 bytes is the remainder of three, of which the reference copies one texel.  The last pitch of the list is
    drawn bottom-up as well."""
    cf = RGB_SOURCES[src]
    c = case(cf, w, 6, (w, 6), 860 + cf + w, 0)
    ps = rgb_pitches(src, cf, w)
    if src == "rgb48" and w == 46:
        assert 288 in ps and rgb_texels_written(src, 288, w) == 46 and rgb_texels_written(src, synth.default_pitch(cf, w), w) == 44
    if src == "rgb24" and w == 47:
        assert rgb_texels_written(src, ps[0], w) == 45 and rgb_texels_written(src, synth.default_pitch(cf, w), w) == 47
    check_layouts(mpcvr, torch_cuda, oracle, c, "rgb", ps + [-ps[1], -ps[-1]], "passes:")


def test_rgb48_fills_the_last_group_at_a_padded_pitch(mpcvr, oracle, torch_cuda):
    """The one divergence the issue names, on its own: RGB48, 46 wide, pitch 288 = 48 * 6 — texels 44 and 45 hold the sample's pixels, in single
    frames and in a batch, as the oracle's widened row has them (oracle/mpcvr_oracle.c: setup_convert, orc_repack_rgb)."""
    torch = torch_cuda
    c = case(33, 46, 6, (46, 6), 890, 0)
    vp, ww, wh = context(mpcvr, c, 288, "default")
    buf, sp = padded_sample(c, 288, POISON_A)
    dev = torch.from_numpy(buf).cuda()
    got = draw(torch, vp, dev, sp, ww, wh)
    assert got[:, 44:46, :3].any(), "the last two texels of the row are black"
    against_oracle(oracle, c, buf, sp, got, "default", "rgb48 46 wide at pitch 288")
    dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
    vp.ProcessBatch([dev, dev, dev], dsts, ww * 4)
    vp.Synchronize()
    for d in dsts:
        assert np.array_equal(d.cpu().numpy(), got), "batch"
    vp.close()


# ---- the same bytes, transported otherwise ------------------------------------------------------------------------------------------------
TRANSPORT = {
    "up2x": (case(2, 136, 24, (272, 48), 900, HDR10, iUpscaling=4), "fused_up2x"),
    "strip": (case(2, 136, 24, (100, 18), 901, SDR, iDownscaling=2), "kernel=fused_strip("),
    "direct": (case(1, 264, 16, (264, 16), 902), "direct:convert"),
    "v210": (case(10, 70, 12, (140, 24), 903, iUpscaling=2), ""),
    "rgb32": (case(30, 46, 12, (69, 18), 904, 0, iUpscaling=2), "passes:source"),
}


@pytest.mark.parametrize("cls", ["wide", "mod8=4"])
@pytest.mark.parametrize("route", sorted(TRANSPORT))
def test_batches_of_padded_samples(mpcvr, oracle, torch_cuda, route, cls):
    """mpcvr_process_batch over three different pictures at a padded pitch == the three single frames, bit for bit; poison A == poison B for the
    batch; every frame against the oracle."""
    torch = torch_cuda
    c0, kernel = TRANSPORT[route]
    pitch = pitch_of(cls, c0["cformat"], c0["w"])
    vp, ww, wh = context(mpcvr, c0, pitch, "default")
    cases = [dict(c0, seed=c0["seed"] + 50 * k) for k in range(3)]
    batches = {}
    for poison in (POISON_A, POISON_B):
        bufs = [padded_sample(c, pitch, poison)[0] for c in cases]
        devs = [torch.from_numpy(b).cuda() for b in bufs]
        singles = [draw(torch, vp, d, pitch, ww, wh) for d in devs]
        info = vp.GetVPInfo()
        assert names(info, kernel), info
        dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
        vp.ProcessBatch(devs, dsts, ww * 4)
        vp.Synchronize()
        outs = [d.cpu().numpy() for d in dsts]
        assert vp.GetLastBatchInfo()["frames"] == 3
        for k in range(3):
            assert np.array_equal(outs[k], singles[k]), f"{route} <{cls}: pitch {pitch}> frame {k} of the batch differs from the single frame [{info}]"
            if poison == POISON_A:
                against_oracle(oracle, cases[k], bufs[k], pitch, outs[k], "default", f"{route} <{cls}: pitch {pitch}> batch frame {k} [{info}]")
        assert not np.array_equal(outs[0], outs[1])
        batches[poison] = outs
    vp.close()
    for k in range(3):
        assert np.array_equal(batches[POISON_A][k], batches[POISON_B][k]), f"{route} <{cls}> batch frame {k} depends on the padding bytes"


HOST_ROUTES = {"up2x": TRANSPORT["up2x"][0], "direct": TRANSPORT["direct"][0], "yv12_strip": case(14, 136, 24, (204, 36), 905, iUpscaling=4),
               "v210": TRANSPORT["v210"][0], "rgb24": case(29, 46, 12, (46, 12), 906, 0)}


@pytest.mark.parametrize("cls", ["wide", "mod4=2"])
@pytest.mark.parametrize("route", sorted(HOST_ROUTES))
def test_host_and_pinned_samples_at_a_padded_pitch(mpcvr, oracle, torch_cuda, route, cls):
    """MPCVR_MEM_HOST and MPCVR_MEM_HOST_PINNED carry pitch * lines bytes through the upload ring: == the device sample, bit for bit (which is held
    to the oracle).  v210 has no pitch of 2 mod 4: its second class is the merely 4-aligned pitch."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = HOST_ROUTES[route]
    pitch = pitch_of(cls, c["cformat"], c["w"]) or row_bytes(c["cformat"], c["w"]) + 4
    buf, sp = padded_sample(c, pitch, POISON_A)
    vp, ww, wh = context(mpcvr, c, pitch, "default")
    want = draw(torch, vp, torch.from_numpy(buf).cuda(), sp, ww, wh)
    info = vp.GetVPInfo()
    against_oracle(oracle, c, buf, sp, want, "default", f"{route} <{cls}: pitch {pitch}> device sample [{info}]")
    host = draw(torch, vp, buf.copy(), sp, ww, wh, mem_kind=api.MEM_HOST)
    assert np.array_equal(host, want), f"{route} <{cls}: pitch {pitch}> host sample [{info}]"
    pin = torch.empty(buf.size, dtype=torch.uint8).pin_memory()
    pin.numpy()[:] = buf
    pinned = draw(torch, vp, pin, sp, ww, wh, mem_kind=api.MEM_HOST_PINNED)
    assert np.array_equal(pinned, want), f"{route} <{cls}: pitch {pitch}> pinned sample [{info}]"
    assert vp.GetVPInfo() == info
    vp.close()


@pytest.mark.parametrize("cls", ["wide", "mod4=2"])
@pytest.mark.parametrize("route", ["up2x", "direct", "yv12_strip"])
def test_device_sample_two_bytes_off_a_dword(mpcvr, oracle, torch_cuda, route, cls):
    """A device sample at +2: copied into the context's texture as pitch * lines bytes first (PrepareSample) == the aligned sample, bit for bit."""
    torch = torch_cuda
    c = HOST_ROUTES[route]
    pitch = pitch_of(cls, c["cformat"], c["w"])
    buf, sp = padded_sample(c, pitch, POISON_B)
    vp, ww, wh = context(mpcvr, c, pitch, "default")
    want = draw(torch, vp, torch.from_numpy(buf).cuda(), sp, ww, wh)
    info = vp.GetVPInfo()
    against_oracle(oracle, c, buf, sp, want, "default", f"{route} <{cls}: pitch {pitch}> aligned sample [{info}]")
    big = torch.zeros(buf.size + 64, dtype=torch.uint8, device="cuda")
    big[2:2 + buf.size] = torch.from_numpy(buf).cuda()
    sample = big[2:2 + buf.size]
    assert sample.data_ptr() % 4 == 2
    got = draw(torch, vp, sample, sp, ww, wh)
    assert np.array_equal(got, want), f"{route} <{cls}: pitch {pitch}> sample at +2 [{info}]"
    vp.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def hr_of(api, fn):
    with pytest.raises(api.MpcvrError) as e:
        fn()
    return e.value.hr


def test_tight_pitch_on_a_padded_context_is_refused_and_the_sample_stays(mpcvr, oracle, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    c = TRANSPORT["up2x"][0]
    pitch = pitch_of("wide", c["cformat"], c["w"])
    t_pitch = synth.default_pitch(c["cformat"], c["w"])
    vp, ww, wh = context(mpcvr, c, pitch, "default")
    assert vp.GetFrameBytes() == (pitch * c["h"] * 3 // 2, pitch)
    buf, sp = padded_sample(c, pitch, POISON_A)
    other = padded_sample(dict(c, seed=c["seed"] + 1), t_pitch, None)[0]
    dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
    vp.CopySample(torch.from_numpy(buf).cuda(), sp)
    assert hr_of(api, lambda: vp.CopySample(torch.from_numpy(other).cuda(), t_pitch)) == api.E_UNEXPECTED
    assert hr_of(api, lambda: vp.CopySample(other, t_pitch, mem_kind=api.MEM_HOST)) == api.E_UNEXPECTED
    vp.Process(dst, ww * 4)
    vp.Synchronize()
    against_oracle(oracle, c, buf, sp, dst.cpu().numpy(), "default", "the sample handed over before the refusals")
    vp.close()


@pytest.mark.parametrize("cformat", [20, 21, 22, 23])
def test_odd_chroma_pitch_of_16_bit_planes_is_refused(mpcvr, torch_cuda, cformat):
    """YUV420P10/16, YUV422P10/16: a luma pitch of 2 mod 4 would start 16-bit chroma rows on odd addresses (pitch // 2 is odd) — no decoder lays a
    frame out that way; mpcvr_set_input answers E_INVALIDARG (include/mpcvr.h) and leaves the context as it was."""
    from videorenderer_amd import api
    vp = api.VideoProcessor(api.default_settings())
    w, h = 70, 10
    vp.InitMediaType(cformat, w, h, pitch=144)
    assert vp.GetFrameBytes()[1] == 144
    for bad in (142, 146, 2 * w + 2):
        assert hr_of(api, lambda: vp.InitMediaType(cformat, w, h, pitch=bad)) == api.E_INVALIDARG, bad
        assert vp.GetFrameBytes()[1] == 144
    vp.InitMediaType(cformat, w, h, pitch=2 * w)        # (the tight pitch of an even width is a multiple of 4)
    vp.close()


def test_zz_route_log(torch_cuda):
    """Not a check: prints which kernel every (route, format, pitch class) of this module ran (pytest -s)."""
    for row in ROUTE_LOG:
        print("ROUTE", *row, sep="\t")
