"""Which BITS of a sample reach a pixel (tests/sample_bits.py builds the samples; tests/test_sample_bits.py shows on the CPU that the oracle
ignores the `high`, `alpha` and `pad` bits of every format and reads the `low` bits of P010 / P210 / Y210).

For every (route, format) one context per tier draws seven samples of the same size:
  (a) a legal noise frame and its two with_ignored_bits twins give the same frame bit for bit, on the default tier and on the plain tier
      (MPCVR_FLAG_NO_FUSED): a difference is an ignored bit that reached a pixel — the message names the first differing pixel's source words;
  (b) container_noise (every bit of every word random: LSB-aligned 10-bit words 0 .. 65535, alpha and pad set) and corner_frame (0, 1, the
      legal range's ends and their neighbours, max - 1, max, and 1023 / 1024 / 1025 / 0xFC00 / 0xFFFF where words wrap) against
      oracle.process on the same bytes at the bars of tests/test_parity_gpu.py: the plain tier exact, with or without a tail; the other tiers
      `compare` (<= 1 code, >= 99 % identical) where there is no tail, and behind a PQ / HLG / Dolby Vision tail sparse_edges (legal noise,
      every 7th sample a corner value) through compare_behind_tail with its defaults (an R10G10B10A2 target: in ten-bit codes);
  (c) not vacuous: with_low_bits changes the frame on P010 / P210 / Y210, on every tier; more than 90 % of the container_noise words of an
      LSB-aligned 10-bit format are >= 1024;
  (d) GetVPInfo names the route the case is meant for (the plain tier: "passes:").
The other ways in — host memory, batches, a v210 row whose last group has fields past the width — at the end.

CopyPlane10to16 (Helper.cpp:789-803) is why a word of 1024 + k must read as k: the fused loaders used to hand the raw word to a matrix that
carried 2^6 / 65535, so (a) failed on every fused route of YUV420P10 / 422P10 / 444P10, GBRP10 and Y10 with the plain tier passing.
"""
import numpy as np
import pytest

from tests.golden.cases import HDR10, HLG, case_frame, oracle_params
from tests.sample_bits import LSB10, MSB10, SEEDS, container_noise, corner_frame, first_difference, sparse_edges, with_ignored_bits, with_low_bits
from tests.sample_layouts import pitch_of, relayout
from tests.test_parity_gpu import BG, compare_behind_tail, compare_rgb10, has_tail       # (make_vp, compare, path_ok: through context / against_oracle / names)
from tests.test_sample_layout_gpu import SDR, UP2X_SOURCES, against_oracle, case, context, direct_kernel, draw, names
from videorenderer_amd import synth

pytestmark = pytest.mark.gpu

TIERS = ("default", "plain")
ROUTE_LOG = []          # (route, format, tier, info): printed at the end of the module (pytest -s / a job script's log)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def samples_of(c, pitch=None):
    """the case's seven samples at `pitch` (default: synth's): legal, twin A, twin B, low bits, container noise, corners, sparse edges"""
    cf, w, h = c["cformat"], c["w"], c["h"]
    legal, tight = case_frame(dict(c, bottom_up=0, pitch=None))
    noise, _ = container_noise(cf, w, h, c["seed"])
    corner, _ = corner_frame(cf, w, h)
    if cf in LSB10:
        assert (noise.view("<u2") >= 1024).mean() > 0.9                                                   # (c), on the input
    out = dict(legal=legal, twin_a=with_ignored_bits(legal, cf, w, h, SEEDS[0]), twin_b=with_ignored_bits(legal, cf, w, h, SEEDS[1]),
               low=with_low_bits(legal, cf, w, h, SEEDS[0]), noise=noise, corner=corner, sparse=sparse_edges(legal, cf, w, h))
    if pitch is not None and pitch != tight:
        out = {k: relayout(v, cf, w, h, pitch, None) for k, v in out.items()}
    return out, (tight if pitch is None else pitch)


def to_oracle(oracle, c, sample, pitch, got, tier, what):
    """(b): against_oracle of the layout tests; an R10G10B10A2 target is compared in its own ten-bit codes — the plain tier exact, the other
    tiers behind a tail through compare_behind_tail(ten_bit=True) with its defaults (one ten-bit code, >= 99 % identical)"""
    if c.get("output_format", 0) != 1:
        return against_oracle(oracle, c, sample, pitch, got, tier, what)
    p = oracle_params(oracle, c)
    want = oracle.process(p, sample, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    if tier == "plain" or not has_tail(c):
        compare_rgb10(got, want, what, exact=tier == "plain")
    else:
        compare_behind_tail(oracle, p, sample, pitch, got, want, what, ten_bit=True)


def check_bits(mpcvr, torch, oracle, c, route, kernel, pitch=None, default_is_exact=False):
    """default_is_exact: the default tier runs no fused kernel on the case (the convert-less resize passes, which keep the plain kernels'
    arithmetic) and is held to the oracle's bits like the plain tier"""
    cf, w, h = c["cformat"], c["w"], c["h"]
    s, pitch = samples_of(c, pitch)
    for tier in TIERS:
        vp, ww, wh = context(mpcvr, c, pitch, tier)
        out = {k: draw(torch, vp, torch.from_numpy(v).cuda(), pitch, ww, wh) for k, v in s.items()}
        info = vp.GetVPInfo()
        vp.close()
        ROUTE_LOG.append((route, cf, tier, info))
        what = f"{route} cformat {cf} {w}x{h} -> {c['dst']} <{tier}> [{info}]"
        # (d)
        assert info.startswith("passes:") if tier == "plain" else names(info, kernel), f"{what}: expected {kernel}"
        # (a)
        for twin in ("twin_a", "twin_b"):
            assert np.array_equal(out[twin], out["legal"]), (f"{what}: {int((out[twin] != out['legal']).sum())} bytes depend on high / alpha / pad bits ({twin}); "
                                                             + first_difference(out["legal"], out[twin], s[twin], cf, w, h, pitch))
        # (c)
        assert (cf in MSB10) == (not np.array_equal(out["low"], out["legal"])), f"{what}: the bits under the 10-bit code"
        # (b)
        bar = "plain" if default_is_exact else tier
        if default_is_exact:
            assert "kernel=" not in info and not info.startswith("direct:") and not has_tail(c), what
        if bar == "plain" or not has_tail(c):
            to_oracle(oracle, c, s["noise"], pitch, out["noise"], bar, what + " container_noise")
            to_oracle(oracle, c, s["corner"], pitch, out["corner"], bar, what + " corner_frame")
        else:
            to_oracle(oracle, c, s["sparse"], pitch, out["sparse"], tier, what + " sparse_edges")


# ---- exact 2x ------------------------------------------------------------------------------------------------------------------------
# the layout file's sources, and six more: the planner gives each of them k_fused_up2x at 2x (tests/test_parity_gpu.py: the packed 4:2:2,
# packed 4:4:4, planar 4:4:4, GBRP and gray cases "on the fused paths")
UP2X_MORE = {"y210": (8, SDR), "ayuv": (11, SDR), "y416": (13, SDR), "yuv444p10": (24, SDR), "gbrp10": (27, 0), "y10": (38, SDR)}
UP2X_ALL = dict(UP2X_SOURCES, **UP2X_MORE)


@pytest.mark.parametrize("src", sorted(UP2X_ALL))
def test_exact_2x(mpcvr, oracle, torch_cuda, src):
    cf, exfmt = UP2X_ALL[src]
    check_bits(mpcvr, torch_cuda, oracle, case(cf, 136, 24, (272, 48), 1100 + cf, exfmt, iUpscaling=4), "up2x", "fused_up2x")


@pytest.mark.parametrize("src", ["p010", "yuv420p10"])
def test_fused_jinc_2x(mpcvr, oracle, torch_cuda, src):
    cf = {"p010": 2, "yuv420p10": 20}[src]
    check_bits(mpcvr, torch_cuda, oracle, case(cf, 136, 24, (272, 48), 1140 + cf, SDR, iUpscaling=5), "jinc2x", "fused_jinc2x")


# ---- arbitrary ratio -----------------------------------------------------------------------------------------------------------------
STRIP_SOURCES = {"p010": 2, "nv12": 1, "yv12": 14, "yuv420p10": 20}
SURFACE_SOURCES = {"xrgb32": 30, "argb32": 31, "r210": 32, "rgb24": 29, "rgb48": 33, "bgra64": 35, "b64a": 36, "v210": 10}
GEO = {"up_1p5x": (204, 36), "down": (100, 18)}


@pytest.mark.parametrize("geo", sorted(GEO))
@pytest.mark.parametrize("src", sorted(STRIP_SOURCES))
def test_fused_strip(mpcvr, oracle, torch_cuda, src, geo):
    from videorenderer_amd import api
    cf = STRIP_SOURCES[src]
    c = case(cf, 136, 24, GEO[geo], 1160 + cf, SDR, iUpscaling=4, iDownscaling=2, lib_flags=api.FLAG_NO_PERIOD)
    check_bits(mpcvr, torch_cuda, oracle, c, f"strip/{geo}", "kernel=fused_strip(")


@pytest.mark.parametrize("geo", sorted(GEO))
@pytest.mark.parametrize("src", sorted(SURFACE_SOURCES))
def test_fused_strip_from_a_surface(mpcvr, oracle, torch_cuda, src, geo):
    """interleaved RGB: copied / repacked into the context's texture.  The 8-bit and 10-bit textures (RGB24, XRGB32 / ARGB32, r210) feed the
    surface variant of the strip kernel; the 16-bit ones (RGB48, BGRA64, b64a: R16G16B16A16) are no surface it reads and take the resize passes
    on the default tier too, where they are held to the oracle's bits like the plain tier; v210 behind its unpack to Y210 is a Y'CbCr sample again and runs k_fused_strip itself."""
    from videorenderer_amd import api
    cf = SURFACE_SOURCES[src]
    c = case(cf, 136, 24, GEO[geo], 1200 + cf, SDR if cf == 10 else 0, iUpscaling=4, iDownscaling=2, lib_flags=api.FLAG_NO_PERIOD)
    wide = cf in (33, 35, 36)
    kernel = "kernel=fused_strip(" if cf == 10 else "passes:source,resizeX,resizeY+final" if wide else "kernel=fused_strip:surface("
    check_bits(mpcvr, torch_cuda, oracle, c, f"strip:surface/{geo}", kernel, default_is_exact=wide)


@pytest.mark.parametrize("src", ["p010_pq", "nv12", "yuv420p10"])
def test_fused_period_4_3(mpcvr, oracle, torch_cuda, src):
    cf, exfmt = UP2X_SOURCES[src]
    check_bits(mpcvr, torch_cuda, oracle, case(cf, 144, 24, (192, 32), 1240 + cf, exfmt, iUpscaling=4), "period/4:3", "kernel=fused_period(rows=4:3,taps=5,")


# ---- same size ------------------------------------------------------------------------------------------------------------------------
DIRECT = {
    # name: (cformat, extfmt, settings, the kernel behind "direct:convert" at the tight pitch, GetVPInfo)
    "nv12": (1, SDR, {}, "k_convert_stream", "direct:convert"),
    "p010": (2, SDR, {}, "k_convert_stream", "direct:convert"),
    "yuv420p10": (20, SDR, {}, "k_convert_blocks", "direct:convert"),
    "yuv422p10": (22, SDR, {}, "k_convert_blocks", "direct:convert"),
    "p010_hlg": (2, HLG, {}, "k_convert_stream", "direct:convert"),
    "p010_pq_hdr_output": (2, HDR10, dict(hdr_output=1, output_format=1), "k_convert_stream", "direct:convert+copy"),
}


@pytest.mark.parametrize("src", sorted(DIRECT))
def test_direct_convert(mpcvr, oracle, torch_cuda, src):
    cf, exfmt, kw, kernel, info = DIRECT[src]
    assert direct_kernel(cf, 264, 16, synth.default_pitch(cf, 264)) == kernel
    check_bits(mpcvr, torch_cuda, oracle, case(cf, 264, 16, (264, 16), 1260 + cf, exfmt, **kw), f"direct/{kernel}", info)


@pytest.mark.parametrize("src", ["nv12", "yuv420p10"])
def test_per_pixel_convert_at_a_pitch_of_2_mod_4(mpcvr, oracle, torch_cuda, src):
    """NV12: a luma pitch of 2 mod 4; YUV420P10 (whose 16-bit chroma rows need an even chroma pitch): 4 mod 8, a chroma pitch of 2 mod 4 —
    no dword loads on either, the per-pixel kernel converts the frame"""
    cf = {"nv12": 1, "yuv420p10": 20}[src]
    pitch = pitch_of("mod4=2" if cf == 1 else "mod8=4", cf, 264)
    assert direct_kernel(cf, 264, 16, pitch) == "k_convert_direct"
    check_bits(mpcvr, torch_cuda, oracle, case(cf, 264, 16, (264, 16), 1280 + cf, SDR), "direct/k_convert_direct", "direct:convert", pitch=pitch)


# ---- Dolby Vision ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", [(96, 32), (192, 64)])
@pytest.mark.parametrize("curves", ["poly", "mmr"])
def test_dolby_vision_block_convert(mpcvr, oracle, torch_cuda, curves, dst):
    """P010 base layer behind the reshaping curves, same size (the block convert writes the target) and 2x (it feeds the resize): the low
    six bits are set in container_noise and the curves see every pivot's neighbourhood in corner_frame"""
    from tests.golden.cases import GOLDEN_CASES
    c = case(2, 96, 32, dst, 1300 + dst[0], GOLDEN_CASES["dovi_poly_sdr"]["exfmt"], iUpscaling=4, dovi=dict(kind=curves))
    check_bits(mpcvr, torch_cuda, oracle, c, f"dovi/{curves}", "direct:convert+final" if dst == (96, 32) else "passes:convert,resizeX,resizeY+final;kernel=fused_strip:surface(")


# ---- the other ways in ------------------------------------------------------------------------------------------------------------------
OTHER = {"v210": 10, "r210": 32, "rgb48": 33, "rgb24": 29, "yuv420p10": 20}


@pytest.mark.parametrize("src", sorted(OTHER))
def test_host_samples_and_batches_of_container_noise(mpcvr, oracle, torch_cuda, src):
    """136 x 24 -> 204 x 36: the container_noise sample handed over as MPCVR_MEM_HOST (the upload ring and the repack behind it) == the same
    sample as MPCVR_MEM_DEVICE, bit for bit; a batch of three different samples (the batch textures' repack) == the three single frames"""
    from videorenderer_amd import api
    torch = torch_cuda
    cf = OTHER[src]
    c = case(cf, 136, 24, (204, 36), 1400 + cf, 0 if cf in (32, 33, 29) else SDR, iUpscaling=4)
    bufs = [container_noise(cf, 136, 24, c["seed"] + 17 * k) for k in range(3)]
    pitch = bufs[0][1]
    vp, ww, wh = context(mpcvr, c, pitch, "default")
    devs = [torch.from_numpy(b).cuda() for b, _ in bufs]
    singles = [draw(torch, vp, d, pitch, ww, wh) for d in devs]
    info = vp.GetVPInfo()
    ROUTE_LOG.append(("host+batch", cf, "default", info))
    against_oracle(oracle, c, bufs[0][0], pitch, singles[0], "default", f"{src} device sample [{info}]")
    host = draw(torch, vp, bufs[0][0].copy(), pitch, ww, wh, mem_kind=api.MEM_HOST)
    assert np.array_equal(host, singles[0]), f"{src}: the host sample differs from the device sample [{info}]"
    dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
    vp.ProcessBatch(devs, dsts, ww * 4)
    vp.Synchronize()
    assert vp.GetLastBatchInfo()["frames"] == 3
    for k in range(3):
        assert np.array_equal(dsts[k].cpu().numpy(), singles[k]), f"{src}: frame {k} of the batch differs from the single frame [{info}]"
    assert not np.array_equal(singles[0], singles[1])
    vp.close()


def test_v210_row_whose_last_group_has_fields_past_the_width(mpcvr, oracle, torch_cuda):
    """130 = 21 groups of six and four pixels: the last group's two luma and one chroma pair past the width, and bits 30..31 of every dword,
    are set (container_noise) or drawn twice (the twins); both tiers, device and host memory, held to the oracle (k_fused_strip behind the
    unpack to Y210 on the default tier)"""
    from videorenderer_amd import api
    torch = torch_cuda
    c = case(10, 130, 24, (195, 36), 1450, SDR, iUpscaling=4)
    check_bits(mpcvr, torch, oracle, c, "v210/130", "passes:convert,resizeX,resizeY+final;kernel=fused_strip(")
    noise, pitch = container_noise(10, 130, 24, c["seed"])
    for tier in TIERS:
        vp, ww, wh = context(mpcvr, c, pitch, tier)
        dev = draw(torch, vp, torch.from_numpy(noise).cuda(), pitch, ww, wh)
        host = draw(torch, vp, noise.copy(), pitch, ww, wh, mem_kind=api.MEM_HOST)
        dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(3)]
        vp.ProcessBatch([torch.from_numpy(noise).cuda()] * 3, dsts, ww * 4)
        vp.Synchronize()
        info = vp.GetVPInfo()
        vp.close()
        assert np.array_equal(host, dev), f"v210 130 wide <{tier}>: host sample [{info}]"
        for d in dsts:
            assert np.array_equal(d.cpu().numpy(), dev), f"v210 130 wide <{tier}>: batch [{info}]"


def test_zz_route_log(torch_cuda):
    """Not a check: prints which kernel every (route, format, tier) of this module ran (pytest -s)."""
    for row in ROUTE_LOG:
        print("ROUTE", *row, sep="\t")
